"""Where the time of the ragged boxed knn_point and of the ragged knn gradient goes: per-kernel device times (the
library's own event brackets, ms per call) at 8 x 16384 x 8192, k = 16 with the counts of either side ragged, full or uniform.
python tools/experiments/knn_ragged_probe.py"""
import sys
import numpy as np, torch
sys.path.insert(0, __file__.rsplit('/', 3)[0])
from rfnet_amd import _raw
from rfnet_amd._lib import profile_collect, profile_enable
def cuda(a): return torch.from_numpy(np.ascontiguousarray(a)).cuda()
def kernels(fn, reps=10):
    fn(); torch.cuda.synchronize(); profile_enable(True)
    for _ in range(reps): fn()
    torch.cuda.synchronize(); prof = profile_collect(); profile_enable(False)
    return {k: round(v[0] / reps, 4) for k, v in sorted(prof.items())}
rng = np.random.RandomState(100)
b, n, m, k = 8, 16384, 8192, 16
a = cuda(rng.random_sample((b, n, 3)).astype(np.float32)); q = cuda(rng.random_sample((b, m, 3)).astype(np.float32))
l1 = rng.randint(n // 4, n + 1, size=b).astype(np.int32); l2 = rng.randint(m // 4, m + 1, size=b).astype(np.int32)
print('len1', l1, 'len2', l2)
F1, F2 = cuda(np.full(b, n, np.int32)), cuda(np.full(b, m, np.int32))
D1, D2 = cuda(l1), cuda(l2)
for name, x, y in (('full', F1, F2), ('len1 ragged', D1, F2), ('len2 ragged', F1, D2), ('both', D1, D2),
                   ('all n/4', cuda(np.full(b, n // 4, np.int32)), F2), ('all n/2', cuda(np.full(b, n // 2, np.int32)), F2)):
    print('knn boxes', name, kernels(lambda: _raw.knn_point(k, a, q, form='boxes', lengths1=x, lengths2=y)))
print('knn boxes plain', kernels(lambda: _raw.knn_point(k, a, q, form='boxes')))
for nn in (n // 4, n // 2):
    print('knn boxes plain on', nn, 'candidates', kernels(lambda: _raw.knn_point(k, a[:, :nn].contiguous(), q, form='boxes')))
g = cuda(rng.randn(b, m, k).astype(np.float32)); idx = _raw.knn_point(k, a, q)[1]
print('grad plain ', kernels(lambda: _raw.knn_point_grad(a, q, idx, g)))
print('grad full  ', kernels(lambda: _raw.knn_point_grad(a, q, idx, g, lengths1=F1, lengths2=F2)))
print('grad ragged', kernels(lambda: _raw.knn_point_grad(a, q, _raw.knn_point(k, a, q, lengths1=D1, lengths2=D2)[1], g, lengths1=D1, lengths2=D2)))
