#!/usr/bin/env python3
"""Writes tests/golden/procrustes_hp.npz: poses where a Procrustes alignment goes wrong quietly, with both row errors of
zedo_min_mpjpe evaluated in mpmath at 50 digits (tests/_procrustes_ref.py::hp_row) and rounded once to float64.

    python tools/gen_procrustes_reference.py            # writes the fixture (byte-identical on every run: fixed seeds, fixed zip dates)
    python tools/gen_procrustes_reference.py --check    # regenerates in memory and compares with the committed file
    python tools/gen_procrustes_reference.py --report   # the float64 oracle's ratios per family (profiles/procrustes_accuracy.txt)

Every pose has H = 4 hypotheses (four draws of the prediction); the draws are repeated with the next seed until the runner-up is at
least 100 bounds above the minimum under both protocols, so the arg-min can be asserted exactly.

Families (id: construction; joint counts):
 1 ordinary: gt sigma = 0.3 m root-centred, pred = gt + 5 cm noise; 3, 4, 5, 16, 17, 21, 64 joints, two poses each
 2 mirrored: pred = gt reflected through a random plane + 5 cm noise (det < 0); 4, 17
 3 similar: pred = fp32(s gt Q + t), Q a random rotation, s = 1e-3, 1, 1.7, 1e3: the error is the fp32 rounding, ~1e-8 m; 4, 17, 64
 4 units and offset: pred in millimetres, both sets shifted by (3e3, -2e3, 5e3) m; 17
 5 equal singular values: octahedron +-a e1, +-a e2, +-b e3 (6) and cube corners (8); pred = gt turned by exactly 90 degrees about a
   coordinate axis, by a random Q (noise 0 and 1e-3), and sheared symmetrically in the plane of the two equal axes (M symmetric with
   an equal diagonal: zeta == 0, a 45 degree Jacobi rotation).  In a noise-0 pose only hypothesis 0 is noiseless (the others carry
   1e-4 h of noise): four exact copies would tie.
 6 flatness ladder: third principal axis of gt AND of pred scaled by f = 1e-2, 1e-4, 1e-6, 3e-7, 1e-7, 3e-8, 1e-8, 1e-10, 1e-13, 1e-16, 0, random orientation (f = 0: the normal on a
   coordinate axis, or the coordinates could not be exactly planar), in-plane noise 5 cm; plus gt thin (1e-10) with pred thick and the
   reverse.  17 joints on every rung, 4 joints on 1e-2, 1e-7, 3e-8 and 0.
 7 needle ladder: two principal axes scaled by f (towards rank 1); the same rungs and joint counts
 8 uncorrelated: pred drawn independently of gt; one row with a single joint 1e3 m away; 17
sigma3 of M scales as the product of the two thicknesses and the fp32 prediction is never thinner than its own rounding (~1e-8), so
the ladders cross the kernel's 1e-14 rank test near f = 1e-7."""
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _procrustes_ref as PR  # noqa: E402

H = PR.H
LADDER = [1e-2, 1e-4, 1e-6, 3e-7, 1e-7, 3e-8, 1e-8, 1e-10, 1e-13, 1e-16, 0.0]
LADDER_J4 = [1e-2, 1e-7, 3e-8, 0.0]
OFFSET = np.array([3e3, -2e3, 5e3])
JMAX = 64


def rot(g):
    q, r = np.linalg.qr(g.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def axis_frame(g):
    """An orthogonal matrix that turns about z, then permutes the axes: what was exactly 0 along z (or along y and z) stays exactly 0."""
    a = g.uniform(0, 2 * np.pi)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    return rz @ np.eye(3)[g.permutation(3)]


def rot90(axis):
    m = np.zeros((3, 3))
    a, b = (axis + 1) % 3, (axis + 2) % 3
    m[axis, axis], m[a, b], m[b, a] = 1, -1, 1
    return m


def cases():
    """(family, joint count, tag, builder): builder(g) -> gt [J,3] float64, [H] predictions [J,3] (rounded to fp32 by the caller)."""
    out = []
    centred = lambda g, J: (lambda a: a - a[0:1])(0.3 * g.standard_normal((J, 3)))
    noisy = lambda g, a, sd=0.05: a + sd * g.standard_normal(a.shape)

    def f1(J):
        def b(g):
            gt = centred(g, J)
            return gt, [noisy(g, gt) for _ in range(H)]
        return b
    for J in (3, 4, 5, 16, 17, 21, 64):
        out += [(1, J, f"ordinary-{k}", f1(J)) for k in range(2)]

    def f2(J):
        def b(g):
            gt = centred(g, J)
            n = g.standard_normal(3)
            n /= np.linalg.norm(n)
            return gt, [noisy(g, gt - 2 * np.outer(gt @ n, n)) for _ in range(H)]
        return b
    out += [(2, J, "mirrored", f2(J)) for J in (4, 17)]

    def f3(J, s):
        def b(g):
            gt = centred(g, J)
            return gt, [s * (gt @ rot(g)) + s * 0.5 * g.standard_normal(3) for _ in range(H)]
        return b
    out += [(3, J, f"similar-s{s:g}", f3(J, s)) for J in (4, 17, 64) for s in (1e-3, 1.0, 1.7, 1e3)]

    def f4(g):
        gt = centred(g, 17)
        return gt + OFFSET, [1000.0 * (noisy(g, gt) + OFFSET) for _ in range(H)]
    out += [(4, 17, f"mm-offset-{k}", f4) for k in range(2)]

    octa = np.array([[.25, 0, 0], [-.25, 0, 0], [0, .25, 0], [0, -.25, 0], [0, 0, .5], [0, 0, -.5]])
    cube = 0.25 * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float)

    def f5(shape, kind, sd):
        def b(g):
            preds = []
            for h in range(H):
                if kind == "rot90":
                    p = shape @ rot90((2 + h) % 3).T
                elif kind == "randq":
                    p = shape @ rot(g)
                else:                                               # shear: x <- x + k y, y <- y + k x, k = 2^-(1 + h)
                    k = 2.0 ** -(1 + h)
                    p = shape @ np.array([[1, k, 0], [k, 1, 0], [0, 0, 1.0]])
                level = sd if sd > 0 else 1e-4 * h
                preds.append(p + level * g.standard_normal(p.shape) if kind != "shear" else p)
            return shape.copy(), preds
        return b
    for name, shape in (("octahedron", octa), ("cube", cube)):
        out += [(5, len(shape), f"{name}-{kind}-noise{sd:g}", f5(shape, kind, sd)) for kind in ("rot90", "randq") for sd in (0.0, 1e-3)]
        out.append((5, len(shape), f"{name}-shear", f5(shape, "shear", 0.0)))

    def thin(J, axes, fg, fp):
        """gt and pred drawn in the principal frame, the axes `axes` scaled by fg (gt) and fp (pred), then turned into a random frame."""
        def b(g):
            base = 0.3 * g.standard_normal((J, 3))
            base -= base.mean(0)
            frame = axis_frame(g) if 0.0 in (fg, fp) else rot(g)
            sg, sp = np.ones(3), np.ones(3)
            sg[axes], sp[axes] = fg, fp
            return (base * sg) @ frame, [(noisy(g, base) * sp) @ frame for _ in range(H)]
        return b
    for fam, axes, name in ((6, [2], "flat"), (7, [1, 2], "needle")):
        out += [(fam, 17, f"{name}-f{f:g}", thin(17, axes, f, f)) for f in LADDER]
        out += [(fam, 4, f"{name}-f{f:g}", thin(4, axes, f, f)) for f in LADDER_J4]
    for J in (4, 17):
        out += [(6, J, "flat-gt-thin-pred-thick", thin(J, [2], 1e-10, 1.0)), (6, J, "flat-gt-thick-pred-thin", thin(J, [2], 1.0, 1e-10))]

    def f8(far):
        def b(g):
            preds = [0.3 * g.standard_normal((17, 3)) for _ in range(H)]
            if far:
                preds[1][5, 0] += 1e3
            return centred(g, 17), preds
        return b
    out += [(8, 17, "uncorrelated-0", f8(False)), (8, 17, "uncorrelated-1", f8(False)), (8, 17, "uncorrelated-far-joint", f8(True))]
    return out


def generate(log=None):
    all_cases = cases()
    P = len(all_cases)
    R = P * H
    fx = dict(pred=np.zeros((R, JMAX, 3), np.float32), gt=np.zeros((P, JMAX, 3), np.float64), J=np.zeros(R, np.int32),
              pose_J=np.zeros(P, np.int32), err_p1_hp=np.zeros(R), err_p2_hp=np.zeros(R), sigma=np.zeros((R, 3)), s=np.zeros(R),
              C=np.zeros(R), t=np.zeros(R), t1=np.zeros(R), family=np.zeros(R, np.int32), pose_family=np.zeros(P, np.int32), pose=np.zeros(R, np.int32),
              hyp=np.zeros(R, np.int32), draw=np.zeros(P, np.int32), tag=np.array([c[2] for c in all_cases]))
    for p, (fam, J, tag, build) in enumerate(all_cases):
        for draw in range(20):
            g = np.random.Generator(np.random.Philox(key=[77, 1000 * p + draw]))
            gt, preds = build(g)
            preds = [np.asarray(x, np.float32) for x in preds]
            rows = [PR.hp_row(x, gt) for x in preds]
            e1, e2 = np.array([r["e1"] for r in rows]), np.array([r["e2"] for r in rows])
            b1 = np.array([PR.bound_p1(r["C"], J, r["e1"]) for r in rows])
            b2 = np.array([PR.bound_p2(r["C"], J, r["e2"], r["sigma"], r["t"], r["t1"]) for r in rows])
            if all(np.sort(e)[1] - np.sort(e)[0] >= 100 * b.max() for e, b in ((e1, b1), (e2, b2))):
                break
        else:
            raise SystemExit(f"pose {p} ({tag}, J = {J}): no draw separates the runner-up from the minimum by 100 bounds")
        if log:
            log(f"pose {p:2d} F{fam} J{J:2d} {tag:28s} draw {draw} sigma3/sigma1 {rows[0]['sigma'][2] / rows[0]['sigma'][0]:.1e}")
        fx["gt"][p, :J], fx["pose_J"][p], fx["pose_family"][p], fx["draw"][p] = gt, J, fam, draw
        for h, (x, r) in enumerate(zip(preds, rows)):
            i = p * H + h
            fx["pred"][i, :J] = x
            fx["J"][i], fx["family"][i], fx["pose"][i], fx["hyp"][i] = J, fam, p, h
            fx["err_p1_hp"][i], fx["err_p2_hp"][i], fx["sigma"][i] = r["e1"], r["e2"], r["sigma"]
            fx["s"][i], fx["C"][i], fx["t"][i], fx["t1"][i] = r["s"], r["C"], r["t"], r["t1"]
    ratio = fx["sigma"][:, 2] / fx["sigma"][:, 0]
    for fam in (6, 7):                                              # the ladders stand on both sides of the kernel's rank test
        lad = ratio[fx["family"] == fam]
        assert (lad > 1e-14).any() and (lad < 1e-14).any() and ((lad > 1e-16) & (lad < 1e-12)).any(), (fam, np.sort(lad))
    assert R <= 320
    return fx


def to_bytes(fx):
    """A .npz with fixed member dates, deflated: the same arrays give the same bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(fx):
            m = io.BytesIO()
            np.lib.format.write_array(m, np.ascontiguousarray(fx[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, m.getvalue())
    return buf.getvalue()


def report(fx):
    """The oracle's needed ratios per family -> text."""
    e1, e2 = PR.oracle_rows(fx)
    r1, r2 = PR.needed_ratios(fx, e1, e2)
    b1, b2 = PR.row_bounds(fx)
    lines = ["family | rows | oracle max |d P1| | needs c1 >= | oracle max |d P2| | needs c2 >= | largest P2 bound | P2 bounds < 1e-12"]
    for fam in sorted(PR.FAMILIES):
        m = fx["family"] == fam
        lines.append(f"F{fam} {PR.FAMILIES[fam]} | {int(m.sum())} | {np.abs(e1 - fx['err_p1_hp'])[m].max():.2e} | {r1[m].max():.3f} | "
                     f"{np.abs(e2 - fx['err_p2_hp'])[m].max():.2e} | {r2[m].max():.3f} | {b2[m].max():.2e} | {int((b2[m] < 1e-12).sum())}")
    lines.append(f"all | {len(r1)} | {np.abs(e1 - fx['err_p1_hp']).max():.2e} | {r1.max():.3f} | {np.abs(e2 - fx['err_p2_hp']).max():.2e} | "
                 f"{r2.max():.3f} | {b2.max():.2e} | {int((b2 < 1e-12).sum())}")
    lines.append(f"c1 = 8 x {PR.ORACLE_RATIO_P1} = {PR.C1}, c2 = 8 x {PR.ORACLE_RATIO_P2} = {PR.C2} (tests/_procrustes_ref.py)")
    return "\n".join(lines)


def main():
    if "--report" in sys.argv:
        print(report(PR.load()))
        return 0
    blob = to_bytes(generate(log=print if "-v" in sys.argv else None))
    if "--check" in sys.argv:
        same = open(PR.FIXTURE, "rb").read() == blob
        print("the committed fixture is reproduced byte for byte" if same else "the committed fixture DIFFERS from a fresh run")
        return 0 if same else 1
    with open(PR.FIXTURE, "wb") as f:
        f.write(blob)
    print(f"{PR.FIXTURE}: {len(blob)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
