"""The --select table of run/_select.py against what is derived from it: the parser's choices, check_select_args (the defaults an entry
declares are the ones filled in, a switch it does not declare is refused), the --eval label and help sentence of every selecting entry,
and the --prune refusal.  No GPU and no built library: the table, the parser and the checks import neither."""
import pytest

from run._driver import build_parser, check_select_args
from run._select import MODES, NONE, SWITCHES, prune_refusal

NAMES = ("none", "reproj", "joints", "temporal", "joints-temporal", "joints-fused", "joints-tree", "joints-tree-fused")
VALUE = dict(bone="3", accel="3", temperature="3", smooth="3", seq_len="3")          # a valid value of every switch


def test_the_tables_names_in_order_are_the_parsers_choices():
    assert tuple(MODES) == NAMES and all(MODES[n].name == n for n in NAMES) and MODES[NONE.name] is NONE
    for inference in (False, True):
        action = next(a for a in build_parser("t", inference=inference)._actions if a.dest == "select")
        assert tuple(action.choices) == NAMES and action.default == "none"
    assert [s[0] for s in SWITCHES] == ["bone", "accel", "temperature", "smooth", "seq_len"] and set(VALUE) == {s[0] for s in SWITCHES}


@pytest.mark.parametrize("name", NAMES)
def test_an_entrys_switches_are_filled_and_the_others_refused(name):
    mode, p = MODES[name], build_parser("t", inference=True)
    assert set(mode.switches) <= set(VALUE)
    a = p.parse_args(["--config", "c.py", "--select", name])
    assert a.select == name
    check_select_args(a)
    for switch in VALUE:                                  # exactly the declared defaults; every other switch stays None
        assert getattr(a, switch) == mode.switches.get(switch), switch
    for switch, refusal, _ in SWITCHES:
        a = p.parse_args(["--config", "c.py", "--select", name, "--" + switch, VALUE[switch]])
        if switch in mode.switches:
            check_select_args(a)
            assert getattr(a, switch) == 3
        else:
            with pytest.raises(SystemExit) as e:
                check_select_args(a)
            assert str(e.value) == refusal


@pytest.mark.parametrize("name", NAMES)
def test_an_entry_has_its_label_its_help_sentence_and_its_prune_flag(name):
    mode = MODES[name]
    if name == "none":                                    # selects nothing: no function, nothing to print or to describe
        assert mode.fn is None and mode.label is None and mode.help is None
    else:
        assert callable(mode.fn) and mode.label and mode.help.startswith(name + " = ")
        assert mode.help in build_parser("t", inference=True)._option_string_actions["--select"].help
    assert mode.prune is (name in ("none", "reproj"))
    words = prune_refusal(name)
    if mode.prune:
        assert words is None
    else:
        assert words.startswith(f"--prune with --select {name} is not supported yet")
