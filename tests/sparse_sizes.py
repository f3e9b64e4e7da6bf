"""The size ladder and the input families of the sparse voxel tests above 1100 rows, shared by the GPU and the host tests of the
submanifold and of the strided convolution.  Not a test module itself.

The ladder is the smallest n that reaches each size P of the shared LDS sort (lds_sort.hpp: P is the sample's own count rounded
up to a power of two, the launch is sized from the padded n), and the contract's limit:

    n      threads  P of the counts [n, n // 2 - 1, n // 4, 77]    what else changes at this n
    2049   1024     4096, 1024, 512, 128     (two-stride passes)   4 words a thread at full width; a third chunk of 1024 rows
    4097   512      8192, 2048, 1024, 128    (four-stride passes   16 words a thread; the head scan of the stride map takes 16
                                             with their r == 3     steps of 512 over its two-deep totals; 5 chunks
                                             and r == 1 remainders)
    8193   1024     16384, 4096, 2048, 128   (four-stride)         16 steps of 1024 with all 16 waves; 9 chunks
    16384  1024     16384, 8192, 4096, 128                         row numbers fill the 16-bit field up to 16383; 16 chunks;
                                                                   512 fan-out tiles where every row has its own coarse cell

so every sort size from 128 to 16384 runs, and all but the largest run under a launch sized for a larger one, which is what a
ragged batch does.  A kernel change that moves one of these thresholds moves the rung with it."""
import numpy as np

I32 = np.int32
SIZES = (2049, 4097, 8193, 16384)
FAMILIES = ("lattice", "spread", "cube", "one")


def counts_at(n):
    """the ragged counts of a batch of four at size n: the full size, just below a half, a quarter, 77"""
    return np.array([n, n // 2 - 1, n // 4, 77], I32)


def lattice(rng, n):
    """(n, 3): n distinct cells of a dense 32 x 32 x 16 block round the origin, in a shuffled order"""
    p = rng.permutation(16384)[:n]
    return np.stack([p % 32 - 16, (p // 32) % 32 - 16, p // 1024 - 8], 1)


def family(kind, n, seed, b=4):
    """(b, n, 3) int32, n <= 16384.  "lattice": every row live, most of the 27 slots present; "spread": 2 * lattice + a random
    child slot, every row alone in its coarse cell; "one": every row in the same cell (one live row per sample)"""
    rng = np.random.RandomState(seed)
    if kind == "lattice":
        return np.stack([lattice(rng, n) for _ in range(b)]).astype(I32)
    if kind == "spread":
        return np.stack([2 * lattice(rng, n) + rng.randint(0, 2, (n, 3)) for _ in range(b)]).astype(I32)
    if kind == "one":
        return np.broadcast_to(rng.randint(-9, 9, (b, 1, 3)), (b, n, 3)).astype(I32)
    raise KeyError(kind)
