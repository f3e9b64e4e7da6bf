"""One guarded allocation per C-ABI call: every buffer of the call sits at an exact byte length and a chosen
residue (mod 256) inside a single uint8 tensor, with at least GAP guard bytes on both sides.  What the call may
write (`out`, `scratch`, `inout`) is known, so after the call every other byte -- guards, gaps, inputs -- must be
what it was.  A plain module (no fixtures): tests/test_memory_contract_host.py checks it on the CPU,
tests/test_gpu_memory_contract.py uses it on the GPU."""
import ctypes as C

import numpy as np
import torch

GUARD = 0xA5
GAP = 1024      # least distance between two buffers, and between a buffer and either end of the allocation
ALIGN = 256
ROLES = ("in", "out", "scratch", "inout")
_NP2T = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


class ArenaError(AssertionError):
    pass


class _Buf:
    __slots__ = ("name", "start", "nbytes", "shape", "dtype", "role", "data")

    @property
    def end(self):
        return self.start + self.nbytes


class Arena:
    def __init__(self, device, poison=0xFF):
        self.device = torch.device(device)
        self.poison = int(poison)
        self.bufs = {}
        self._cursor = 0
        self.mem = None
        self.clone = None

    # ---- layout (host only) ----
    def add(self, name, data_or_shape, dtype, role, residue=0):
        """Register a buffer: `data_or_shape` is an array (copied in before the call) or a shape; `dtype` a numpy
        dtype; the buffer starts at an offset = residue (mod 256) and is exactly its own size long."""
        assert self.mem is None, "add() after build()"
        assert role in ROLES and name not in self.bufs and 0 <= residue < ALIGN
        dt = np.dtype(dtype)
        b = _Buf()
        b.name, b.dtype, b.role = name, dt, role
        if isinstance(data_or_shape, np.ndarray):
            b.data = np.ascontiguousarray(data_or_shape.astype(dt, copy=False))
            b.shape = b.data.shape
        else:
            assert role != "in", "an input needs its data"
            b.data = None
            b.shape = tuple(int(v) for v in np.atleast_1d(data_or_shape))
        b.nbytes = int(np.prod(b.shape, dtype=np.int64)) * dt.itemsize
        start = -(-(self._cursor + GAP) // ALIGN) * ALIGN + residue
        b.start = start
        self._cursor = start + b.nbytes
        self.bufs[name] = b
        return name

    def build(self):
        """Allocate; guard byte everywhere, inputs copied in, outputs and scratch poisoned; then snapshot."""
        total = self._cursor + GAP
        raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=self.device)
        skew = (-raw.data_ptr()) % ALIGN
        self._raw = raw
        self.mem = raw[skew:skew + total]
        assert self.mem.data_ptr() % ALIGN == 0, "arena base is not 256-byte aligned"
        self.mem.fill_(GUARD)
        for b in self.bufs.values():
            if b.nbytes == 0:
                continue
            if b.data is not None:
                src = torch.from_numpy(b.data.reshape(-1).view(np.uint8).copy())
                self.mem[b.start:b.end].copy_(src)
            elif b.role in ("out", "scratch"):
                self.mem[b.start:b.end].fill_(self.poison)
            else:
                raise AssertionError(f"{b.name}: an inout buffer needs data")
        self.snapshot()
        return self

    def snapshot(self):
        self._sync()
        self.clone = self.mem.clone()

    def freeze(self, name):
        """An output of an earlier call that later calls must only read (a sorted-set handle): from here on it is
        checked like an input."""
        self.bufs[name].role = "in"
        self.snapshot()

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # ---- access ----
    def addr(self, name):
        return self.mem.data_ptr() + self.bufs[name].start

    def ptr(self, name):
        """ctypes pointer (None for name None: an optional argument left out)."""
        return None if name is None else C.c_void_p(self.addr(name))

    def nbytes(self, name):
        return self.bufs[name].nbytes

    def view(self, name):
        b = self.bufs[name]
        return self.mem[b.start:b.end].view(_NP2T[b.dtype]).reshape(b.shape)

    def get(self, name):
        """The buffer's contents as a numpy array (a copy)."""
        b = self.bufs[name]
        raw = self.mem[b.start:b.end].cpu().numpy()
        return raw.view(b.dtype).reshape(b.shape).copy()

    def still_poison(self, name):
        b = self.bufs[name]
        return bool((self.mem[b.start:b.end] == self.poison).all())

    # ---- the check ----
    def _nearest(self, off):
        def dist(b):
            return 0 if b.start <= off < b.end else min(abs(off - b.start), abs(off - (b.end - 1)))
        return min(self.bufs.values(), key=dist)

    def check(self, what=""):
        """Every byte outside the out / scratch / inout ranges equals the snapshot."""
        self._sync()
        diff = self.mem != self.clone
        for b in self.bufs.values():
            if b.role != "in":
                diff[b.start:b.end] = False
        if not bool(diff.any()):
            return
        where = torch.nonzero(diff).reshape(-1)
        first, count = int(where[0]), int(where.numel())
        b = self._nearest(first)
        lo, hi = max(0, first - 4), min(int(self.mem.numel()), first + 28)
        found = bytes(self.mem[lo:hi].cpu().numpy().tolist()).hex(" ")
        was = bytes(self.clone[lo:hi].cpu().numpy().tolist()).hex(" ")
        if b.start <= first < b.end:
            place = f"inside '{b.name}' (role {b.role}, which the call must not write)"
        elif first < b.start:
            place = f"{b.start - first} bytes BEFORE the start of '{b.name}' (role {b.role})"
        else:
            place = f"{first - b.end} bytes PAST the end of '{b.name}' (role {b.role})"
        raise ArenaError(
            f"{what}: {count} byte(s) changed outside the buffers the call may write; first at arena offset {first}, "
            f"{place}: offset {first - b.start:+d} from the buffer's start, {first - b.end:+d} from its end "
            f"({b.nbytes} bytes, {b.dtype} {b.shape}, start = {b.start % ALIGN} mod {ALIGN}); bytes from offset {lo}: "
            f"found [{found}] expected [{was}]")
