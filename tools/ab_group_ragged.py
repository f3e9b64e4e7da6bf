"""Ragged batches through sampling, grouping and neighbour search on one GPU: per op, the same seeded inputs timed four ways
(ms per call, hipEvents via torch; the four alternated inside every round, inputs rotated between calls):
  plain    the existing op on the full padded batch (what a caller pays today, wrong results aside),
  full     the ragged op with full counts,
  ragged   the ragged op with counts uniform in [n / 4, n] (for FPS the wanted samples scaled likewise),
  loop     a Python loop of batch-1 calls of the existing op on the unpadded slices (what a caller does today).
Shapes: BASELINE.json configs[2] (32 clouds of 16384 points in the unit cube, 1024 samples, r = 0.1, 32 per ball) for FPS, the
ball query and sample_and_group; 32 x 16384 x 1024 for three_nn; 8 x 16384 x 8192, k = 16 for knn_point.  Every figure is the
median over the rounds with [min .. max] behind it: the spread to hold a difference against.
python tools/ab_group_ragged.py [rounds] [--plain-only]   (--plain-only: the first column alone, for a run against another
build named by RFOPS_LIB, tools/build_variant.py)"""
import sys

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from rfnet_amd import _raw  # noqa: E402

SETS = 3   # input sets rotated between calls
REPS = 5   # calls per version and round


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def counts(rng, b, n):
    return rng.randint(n // 4, n + 1, size=b).astype(np.int32)


def ops(plain_only):
    """-> [(name, {version: [callable per input set]})]; plain_only: nothing of the ragged entries is called while setting up"""
    out = []
    rng = np.random.RandomState(100)
    b, n, m, r, ns = 32, 16384, 1024, 0.1, 32
    xyz = [cuda(rng.random_sample((b, n, 3)).astype(np.float32)) for _ in range(SETS)]
    ln = [counts(rng, b, n) for _ in range(SETS)]
    lo = [np.maximum(1, (ln[s].astype(np.int64) * m) // n).astype(np.int32) for s in range(SETS)]
    full_n, full_m = cuda(np.full(b, n, np.int32)), cuda(np.full(b, m, np.int32))
    dln, dlo = [cuda(v) for v in ln], [cuda(v) for v in lo]
    sl = [[xyz[s][i:i + 1, :ln[s][i]].contiguous() for i in range(b)] for s in range(SETS)]
    out.append((f"farthest_point_sample {b} x {n} -> {m}", {
        "plain": [lambda s=s: _raw.farthest_point_sample(m, xyz[s]) for s in range(SETS)],
        "full": [lambda s=s: _raw.farthest_point_sample(m, xyz[s], lengths=full_n, npoints=full_m) for s in range(SETS)],
        "ragged": [lambda s=s: _raw.farthest_point_sample(m, xyz[s], lengths=dln[s], npoints=dlo[s]) for s in range(SETS)],
        "loop": [lambda s=s: [_raw.farthest_point_sample(int(lo[s][i]), sl[s][i]) for i in range(b)] for s in range(SETS)],
    }))
    new = [_raw.gather_point(xyz[s], _raw.farthest_point_sample(m, xyz[s])) for s in range(SETS)]
    rnew = new if plain_only else [_raw.farthest_point_sample(m, xyz[s], lengths=dln[s], npoints=dlo[s], with_xyz=True)[1]
                                   for s in range(SETS)]
    qsl = [[rnew[s][i:i + 1, :lo[s][i]].contiguous() for i in range(b)] for s in range(SETS)]
    for form in ("boxes", "scan"):
        out.append((f"query_ball_point[{form}] {b} x {n} x {m}, r = {r}, {ns} per ball", {
            "plain": [lambda s=s, form=form: _raw.query_ball_point(r, ns, xyz[s], new[s], form=form) for s in range(SETS)],
            "full": [lambda s=s, form=form: _raw.query_ball_point(r, ns, xyz[s], new[s], form=form, lengths1=full_n,
                                                                  lengths2=full_m) for s in range(SETS)],
            "ragged": [lambda s=s, form=form: _raw.query_ball_point(r, ns, xyz[s], rnew[s], form=form, lengths1=dln[s],
                                                                    lengths2=dlo[s]) for s in range(SETS)],
            "loop": [lambda s=s, form=form: [_raw.query_ball_point(r, ns, sl[s][i], qsl[s][i], form=form) for i in range(b)]
                     for s in range(SETS)],
        }))
    out.append((f"sample_and_group {b} x {n} -> {m}, r = {r}, {ns} per ball", {
        "plain": [lambda s=s: _raw.sample_and_group(m, r, ns, xyz[s]) for s in range(SETS)],
        "full": [lambda s=s: _raw.sample_and_group(m, r, ns, xyz[s], lengths=full_n, npoints=full_m) for s in range(SETS)],
        "ragged": [lambda s=s: _raw.sample_and_group(m, r, ns, xyz[s], lengths=dln[s], npoints=dlo[s]) for s in range(SETS)],
        "loop": [lambda s=s: [_raw.sample_and_group(int(lo[s][i]), r, ns, sl[s][i]) for i in range(b)] for s in range(SETS)],
    }))
    # three_nn: 16384 unknown points per sample against 1024 known ones
    kn = [cuda(rng.random_sample((b, m, 3)).astype(np.float32)) for _ in range(SETS)]
    lk = [counts(rng, b, m) for _ in range(SETS)]
    dlk = [cuda(v) for v in lk]
    ksl = [[kn[s][i:i + 1, :lk[s][i]].contiguous() for i in range(b)] for s in range(SETS)]
    for form in ("boxes", "scan"):
        out.append((f"three_nn[{form}] {b} x {n} x {m}", {
            "plain": [lambda s=s, form=form: _raw.three_nn(xyz[s], kn[s], form=form) for s in range(SETS)],
            "full": [lambda s=s, form=form: _raw.three_nn(xyz[s], kn[s], form=form, lengths1=full_n, lengths2=full_m)
                     for s in range(SETS)],
            "ragged": [lambda s=s, form=form: _raw.three_nn(xyz[s], kn[s], form=form, lengths1=dln[s], lengths2=dlk[s])
                       for s in range(SETS)],
            "loop": [lambda s=s, form=form: [_raw.three_nn(sl[s][i], ksl[s][i], form=form) for i in range(b)]
                     for s in range(SETS)],
        }))
    # knn_point: 8 samples, 16384 candidates, 8192 queries, k = 16
    b2, m2, k = 8, 8192, 16
    cand = [xyz[s][:b2].contiguous() for s in range(SETS)]
    qry = [cuda(rng.random_sample((b2, m2, 3)).astype(np.float32)) for _ in range(SETS)]
    l1 = [ln[s][:b2].copy() for s in range(SETS)]
    l2 = [counts(rng, b2, m2) for _ in range(SETS)]
    d1, d2 = [cuda(v) for v in l1], [cuda(v) for v in l2]
    f1, f2 = cuda(np.full(b2, n, np.int32)), cuda(np.full(b2, m2, np.int32))
    csl = [[cand[s][i:i + 1, :l1[s][i]].contiguous() for i in range(b2)] for s in range(SETS)]
    qs2 = [[qry[s][i:i + 1, :l2[s][i]].contiguous() for i in range(b2)] for s in range(SETS)]
    for form in ("boxes", "scan"):
        out.append((f"knn_point[{form}] {b2} x {n} x {m2}, k = {k}", {
            "plain": [lambda s=s, form=form: _raw.knn_point(k, cand[s], qry[s], form=form) for s in range(SETS)],
            "full": [lambda s=s, form=form: _raw.knn_point(k, cand[s], qry[s], form=form, lengths1=f1, lengths2=f2)
                     for s in range(SETS)],
            "ragged": [lambda s=s, form=form: _raw.knn_point(k, cand[s], qry[s], form=form, lengths1=d1[s], lengths2=d2[s])
                       for s in range(SETS)],
            "loop": [lambda s=s, form=form: [_raw.knn_point(k, csl[s][i], qs2[s][i], form=form) for i in range(b2)]
                     for s in range(SETS)],
        }))
    g = [cuda(rng.randn(b2, m2, k).astype(np.float32)) for _ in range(SETS)]
    idx = [_raw.knn_point(k, cand[s], qry[s])[1] for s in range(SETS)]
    ridx = idx if plain_only else [_raw.knn_point(k, cand[s], qry[s], lengths1=d1[s], lengths2=d2[s])[1] for s in range(SETS)]
    isl = [[ridx[s][i:i + 1, :l2[s][i]].contiguous() for i in range(b2)] for s in range(SETS)]
    gsl = [[g[s][i:i + 1, :l2[s][i]].contiguous() for i in range(b2)] for s in range(SETS)]
    out.append((f"knn_point_grad {b2} x {n} x {m2}, k = {k}", {
        "plain": [lambda s=s: _raw.knn_point_grad(cand[s], qry[s], idx[s], g[s]) for s in range(SETS)],
        "full": [lambda s=s: _raw.knn_point_grad(cand[s], qry[s], idx[s], g[s], lengths1=f1, lengths2=f2) for s in range(SETS)],
        "ragged": [lambda s=s: _raw.knn_point_grad(cand[s], qry[s], ridx[s], g[s], lengths1=d1[s], lengths2=d2[s])
                   for s in range(SETS)],
        "loop": [lambda s=s: [_raw.knn_point_grad(csl[s][i], qs2[s][i], isl[s][i], gsl[s][i]) for i in range(b2)]
                 for s in range(SETS)],
    }))
    return out


def timed(fns):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(REPS):
        fns[r % SETS]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 9
    plain_only = "--plain-only" in sys.argv
    torch.cuda.init()
    print(f"# ragged sampling / grouping / neighbour search A/B on {torch.cuda.get_device_name(0)}: {rounds} rounds of {REPS} "
          f"calls per figure, {SETS} input sets in rotation, ms per call, median [min .. max]; "
          f"library: {_raw.lib._name.rsplit('/', 1)[-1]}")
    for name, versions in ops(plain_only):
        if plain_only:
            versions = {"plain": versions["plain"]}
        for fns in versions.values():  # warm every version on every input set
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        ms = {v: [] for v in versions}
        for _ in range(rounds):
            for v, fns in versions.items():  # the versions alternate inside a round
                ms[v].append(timed(fns))
        print(f"\n## {name}")
        for v, t in ms.items():
            print(f"{v:7s} {np.median(t):9.4f}  [{min(t):.4f} .. {max(t):.4f}]")
        if not plain_only:
            p, f, r, lp = (float(np.median(ms[v])) for v in ("plain", "full", "ragged", "loop"))
            print(f"full - plain {1e3 * (f - p):+.1f} us; ragged / plain {r / p:.2f}; loop / ragged {lp / r:.1f}x")


if __name__ == "__main__":
    main()
