"""The labels, the two float64 references and the criterion that hold the time-bias table of zedo_schedule_create (numpy only).
Shared by tests/test_schedule_ref.py (CPU: the fp32 oracle under the same criterion) and tests/test_schedule_gpu.py.

The table is tbias[s, l, :] = W_l_t SiLU(W_s posemb(label_s) + b_s) + b_l_t + b_l (oracle/zedo_oracle.py time_bias_table).  Its
two dense layers cost about 2.5e-7 at every label; what grows with the label is the conditioning of sin / cos(label * freq) in an
fp32 argument, which the reference model shares.  The criterion therefore takes the float64 table AT THE fp32 ARGUMENT as reference and
allows, beside the project's single-call parity rule, a multiple of what forming that argument in fp32 costs - measured between two
float64 evaluations, never from a kernel."""
import math

import numpy as np

P = 67                                  # as _shared.LS_P: odd and prime, every base row visits every position of a 256-row pad and a 128-row tile
OIL_RANGE = np.linspace(9.99, 99.9, 8)  # the labels of the shipped OIL schedules, 999 * (0.01 .. 0.1)
DENORMAL = 1e-40
NAMED = [0.0, DENORMAL, 1e-3, 0.01, 0.5] + list(OIL_RANGE) + [50.0, 300.0, 523.7, 999.0, 2000.0, -99.9, -999.0]
GROUPS = [("|label| <= 1", 0.0, 1.0), ("1 < |label| <= 100", 1.0, 100.0), ("100 < |label| <= 999", 100.0, 999.0), ("|label| = 2000", 999.0, 2000.0)]
PARITY = 2e-6                           # max |error| <= 2e-6 max(1, max |ref|): test_the_one_tile_reference_against_the_float64_oracle
ARG_FACTOR = 2.0                        # see criterion()


def make_labels():
    """67 distinct finite fp32 labels: NAMED, then 47 drawn log-uniformly in [1e-3, 999] (numpy Philox, key [67, 7])."""
    g = np.random.Generator(np.random.Philox(key=[67, 7]))
    drawn = np.exp(g.uniform(math.log(1e-3), math.log(999.0), P - len(NAMED)))
    lab = np.concatenate([np.array(NAMED, np.float64), drawn]).astype(np.float32)
    assert lab.size == P and np.isfinite(lab).all() and np.unique(lab).size == P
    return lab


LABELS = make_labels()


def group_of(label):
    """Index into GROUPS of a label."""
    m = abs(float(label))
    for i, (_, lo, hi) in enumerate(GROUPS):
        if (m <= hi) and (i == 0 or m > lo):
            return i
    raise ValueError(label)


def _table_from_pe(w64, pe):
    """oracle/zedo_oracle.py time_bias_table behind the embedding, float64."""
    import zedo_oracle as O
    temb = O.silu(O._lin(w64, "shared_time_embed.0", pe))
    names = ["pre_dense"] + [f"b{b}_dense{k}" for b in (1, 2) for k in (1, 2)]
    return np.stack([O._lin(w64, n + "_t", temb) + w64[n + ".bias"][None, :] for n in names], axis=1)


def arg32(labels, label_scale=1.0, embed=512):
    """The argument of sin / cos as posemb_kernel states it: fl32(fl32(t * label_scale) * fl32(exp(fl32(k * emb32)))),
    emb32 = fl32(-ln(10000) / 255) -> [S, embed / 2] float32."""
    f32 = np.float32
    half = embed // 2
    emb32 = f32(-math.log(10000.0) / (half - 1))
    freq = np.exp(np.arange(half, dtype=np.float32) * emb32)
    assert freq.dtype == np.float32
    t = np.asarray(labels, np.float32).reshape(-1) * f32(label_scale)
    return t[:, None] * freq[None, :]


def table64(weights, labels, label_scale=1.0):
    """O.time_bias_table in float64 with float64 weights: the argument and the frequencies formed in float64 -> [S,5,1024]."""
    import zedo_oracle as O
    lab = np.asarray(labels, np.float32).astype(np.float64) * float(np.float32(label_scale))
    return O.time_bias_table(O.cast_weights(weights, np.float64), lab, dtype=np.float64)


def table64_at32(weights, labels, label_scale=1.0):
    """The same table with the argument of sin / cos formed in fp32 as the kernel states it (arg32), then everything in float64."""
    import zedo_oracle as O
    a = arg32(labels, label_scale, weights["shared_time_embed.0.weight"].shape[1]).astype(np.float64)
    return _table_from_pe(O.cast_weights(weights, np.float64), np.concatenate([np.sin(a), np.cos(a)], axis=1))


def per_label(d):
    """max |.| over the 5 x 1024 entries of each label's row."""
    return np.abs(d).reshape(d.shape[0], -1).max(1)


def criterion(weights, labels, label_scale=1.0, arg_term=True):
    """-> (ref [S,5,1024] = table64_at32, bound [S], arg_cost [S]):

        max |tbias[s] - ref[s]| <= PARITY * max(1, max |ref[s]|) + ARG_FACTOR * arg_cost[s],   arg_cost[s] = max |table64[s] - ref[s]|.

    The first term is the single-call parity rule of the dense layers.  The second is for implementations that do not form the
    argument of sin / cos with the very bits of arg32 (arg_term = False drops it: the fp32 numpy oracle shares those bits).
    arg_cost[s] is what the table of label s loses when the argument is formed in fp32 instead of float64: the response of the table
    to an argument that the final fp32 rounding of t * freq moves by at most HALF an ulp of the argument (the roundings inside freq
    come on top and only raise the measured cost).  posemb_kernel takes freq from the device's expf, which may differ from numpy's
    exp by ONE ulp of freq; t * freq then moves by up to one ulp of the argument - twice the half ulp that arg_cost is the response
    to, and the response is linear at this size (an ulp of the largest argument, 2000, is 1.2e-4 rad).  Hence ARG_FACTOR = 2.  Neither
    term is fitted to what a kernel achieves: a table that misses this bound has an expf more than one ulp off numpy's, a sin / cos
    without full range reduction, or wrong dense layers."""
    ref = table64_at32(weights, labels, label_scale)
    arg_cost = per_label(table64(weights, labels, label_scale) - ref)
    bound = PARITY * np.maximum(1.0, per_label(ref))
    if arg_term:
        bound = bound + ARG_FACTOR * arg_cost
    return ref, bound, arg_cost


def group_report(err, bound, labels):
    """Per label group: the achieved maximum, the largest share of the criterion used and the label it is used at."""
    rows = []
    share = err / bound
    for i, (name, _, _) in enumerate(GROUPS):
        sel = np.array([group_of(v) == i for v in labels])
        k = int(np.argmax(np.where(sel, share, -1.0)))
        rows.append(dict(group=name, labels=int(sel.sum()), max_abs=float(err[sel].max()), share=float(share[k]), at_label=float(labels[k]),
                         bound_there=float(bound[k])))
    return rows
