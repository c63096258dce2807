"""CPU: the helpers the GPU tests of the label-free family rest on (tests/_invariance.py, _joint_marginal_ref.hold_marginals), held on
their own: same() is a comparison of bits in every floating dtype, with shape and dtype part of equality; misaligned() returns the
residue it promises; refusal_sweep() raises against an entry point that accepts a NULL, names the wrong error, writes before it refuses or
refuses the control; hold_marginals() raises against a reference moved by twice a bound.  The entry points are plain Python closures over
CPU tensors."""
import math

import numpy as np
import pytest
import torch

from _invariance import BADARG, WORKSPACE, all_same, bits, misaligned, ptr, refusal_sweep, same
from _joint_marginal_ref import chain_reference, hold_marginals, marg_bound, mean_bound, reference, spread_of
from _joint_temporal_ref import case


@pytest.mark.parametrize("dt", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=str)
def test_same_tells_the_signed_zeros_apart(dt):
    a, b = torch.zeros(3, dtype=dt), torch.zeros(3, dtype=dt)
    b[1] = -0.0
    assert torch.equal(a, b) and not same(a, b) and same(a, a.clone()) and same(b, b.clone())
    if dt in (torch.float32, torch.float64):
        an, bn = a.numpy(), b.numpy()
        assert np.array_equal(an, bn) and not same(an, bn) and same(an, an.copy())
    assert bits(a).dtype == {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]


@pytest.mark.parametrize("fdt,idt,quiet,other", [(np.float32, np.int32, 0x7FC00000, 0x7FC00001),
                                                 (np.float64, np.int64, 0x7FF8000000000000, 0x7FF8000000000001)], ids=["f32", "f64"])
def test_same_tells_two_nan_payloads_apart_and_calls_identical_nans_equal(fdt, idt, quiet, other):
    a, b = np.array([1.0, 0.0, 2.0], fdt), np.array([1.0, 0.0, 2.0], fdt)
    a.view(idt)[1], b.view(idt)[1] = quiet, other
    assert np.isnan(a[1]) and np.isnan(b[1])
    assert same(a, a.copy()) and not same(a, b) and not np.array_equal(a, a.copy())                 # by value a NaN equals nothing
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    assert same(ta, ta.clone()) and not same(ta, tb) and all_same([ta, tb], [ta.clone(), tb.clone()]) and not all_same([ta], [ta, tb])


def test_same_rejects_equal_values_of_another_dtype_or_shape():
    a = torch.arange(6, dtype=torch.float32)
    assert not same(a, a.double()) and not same(a, a.view(2, 3)) and not same(a, a.to(torch.int32)) and not same(a, a.numpy())
    assert same(a.to(torch.int32), a.to(torch.int32)) and same(a.view(2, 3), a.clone().view(2, 3))
    n = a.numpy()
    assert not same(n, n.astype(np.float64)) and not same(n, n.reshape(2, 3)) and same(n.astype(np.int32), n.astype(np.int32))


@pytest.mark.parametrize("floats,residue", [(3, 12), (1, 4), (51, 12), (15, 12)])
def test_misaligned_returns_the_promised_residue(floats, residue):
    t = torch.arange(5 * 7 * 3, dtype=torch.float32).view(5, 7, 3)
    m = misaligned(t, floats)
    assert t.data_ptr() % 16 == 0 and m.data_ptr() % 16 == residue and m.is_contiguous() and same(m, t)


# ---- refusal_sweep against entry points with one flaw each ---------------------------------------------------------------------

def entry_point(flaw=None):
    """A stand-in for a raw entry point with inputs (slot 0), a workspace (slot 1) and one output (slot 2): it refuses what the sweep
    tries, writes nothing when it refuses, and runs the control - except for its one flaw."""
    need = 64
    x, ws, out = torch.zeros(8), torch.full((need + 8,), 0x5A, dtype=torch.uint8), torch.full((4,), -7.0)
    ptrs = [ptr(x), ptr(ws), ptr(out)]

    def call(p=ptrs, n=4, lam=1.0, tau=1.0, nbytes=need):
        if flaw == "writes_first" and n <= 0:
            out[0] = 0.0
        if any(q is None for q in p) and not (flaw == "accepts_null" and p[0] is None and None not in p[1:]):
            return BADARG
        if n <= 0 or not (math.isfinite(lam) and lam >= 0) or not (math.isfinite(tau) and tau > 0) or p[1].value % 8:
            return BADARG
        if nbytes < need:
            return BADARG if flaw == "wrong_code" else WORKSPACE
        if flaw == "refuses_the_control":
            return BADARG
        out.fill_(1.0)
        return 0

    kw = dict(sizes=[dict(n=0), dict(n=-3)], weights=("lam",), taus=("tau",), workspace_slot=1, need=need, untouched=((out, -7.0), (ws, 0x5A)))
    return call, ptrs, kw, out


def test_refusal_sweep_passes_an_entry_point_that_keeps_the_contract():
    call, ptrs, kw, out = entry_point()
    refusal_sweep(call, ptrs, (0, 1, 2), **kw)
    assert bool((out == 1.0).all())                                  # the control ran, last


@pytest.mark.parametrize("flaw", ["accepts_null", "wrong_code", "writes_first", "refuses_the_control"])
def test_refusal_sweep_raises_against_a_flawed_entry_point(flaw):
    call, ptrs, kw, _ = entry_point(flaw)
    with pytest.raises(AssertionError):
        refusal_sweep(call, ptrs, (0, 1, 2), **kw)


# ---- hold_marginals against a reference moved by twice a bound -------------------------------------------------------------------

J, N, H, L = 5, 12, 3, 4


def marginals():
    r = reference(J, N, H, L, 100.0, 1.0)
    x, T, _ = case(J, N, H)
    out = [r[k] for k in ("mean", "cov", "hmax", "wmax", "logz", "w")]
    return out, chain_reference(r), dict(beta=marg_bound(L, H, r["G"]), x=x, T=T, N=N)


def test_hold_marginals_passes_the_reference_itself():
    out, ref, kw = marginals()
    seen = hold_marginals(out, **ref, **kw)
    assert seen["e_lw"] <= kw["beta"] and seen["e_mean"] == 0.0 and seen["hmax_differs"] == 0


@pytest.mark.parametrize("what", ["log_w_ref", "logz_ref", "mean_ref"])
def test_hold_marginals_raises_when_the_reference_moves_by_twice_the_bound(what):
    """One log-marginal and one logZ by 2 beta; one coordinate of one mean by twice mean_bound(beta), the bound that quantity is held
    to (2 beta itself is inside it: the bound scales with the largest |X|, about 5 m here)."""
    out, ref, kw = marginals()
    step = 2 * kw["beta"] if what != "mean_ref" else 2 * mean_bound(kw["beta"], spread_of(kw["x"], kw["T"], N)[1])
    assert 0 < step < 1e-9
    moved = ref[what].copy()
    moved[(3, 2, 1)[:moved.ndim]] += step
    assert np.isfinite(moved).all() or what == "log_w_ref"
    with pytest.raises(AssertionError):
        hold_marginals(out, **dict(ref, **{what: moved}), **kw)
