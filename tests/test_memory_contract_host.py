"""CPU: the arena helper of the memory-contract tests checks itself, and the contract's case table covers the ABI."""
import ctypes as C
import fnmatch

import numpy as np
import pytest

from arena import GAP, GUARD, Arena, ArenaError


def _arena():
    A = Arena("cpu", 0x5A)
    A.add("xyz", np.arange(33, dtype=np.float32), np.float32, "in", 4)
    A.add("out", (7, 3), np.float32, "out", 12)
    A.add("ws", (1001,), np.uint8, "scratch", 16)
    A.add("acc", np.ones(5, np.int32), np.int32, "inout", 0)
    return A.build()


def test_arena_layout_and_fill():
    A = _arena()
    assert A.mem.data_ptr() % 256 == 0
    ends = []
    for name, res in (("xyz", 4), ("out", 12), ("ws", 16), ("acc", 0)):
        b = A.bufs[name]
        assert A.addr(name) % 256 == res and b.start >= GAP and A.mem.numel() - b.end >= GAP
        ends.append((b.start, b.end))
    for (_, e0), (s1, _) in zip(ends, ends[1:]):
        assert s1 - e0 >= GAP
    assert A.nbytes("xyz") == 132 and A.nbytes("out") == 84 and A.nbytes("ws") == 1001  # exact, no rounding
    assert np.array_equal(A.get("xyz"), np.arange(33, dtype=np.float32)) and np.array_equal(A.get("acc"), np.ones(5, np.int32))
    assert A.still_poison("out") and A.still_poison("ws")
    assert A.get("out").view(np.uint8).min() == 0x5A
    covered = np.zeros(A.mem.numel(), bool)
    for b in A.bufs.values():
        covered[b.start:b.end] = True
    assert (A.mem.numpy()[~covered] == GUARD).all()
    assert C.cast(A.ptr("xyz"), C.POINTER(C.c_float))[32] == 32.0  # the raw address is the buffer
    assert A.ptr(None) is None


def test_arena_accepts_writes_where_the_call_may_write():
    A = _arena()
    A.view("out").fill_(1.0)
    A.view("ws").fill_(3)
    A.view("acc").add_(2)
    A.check("legal writes")
    assert np.array_equal(A.get("acc"), np.full(5, 3, np.int32)) and not A.still_poison("out")


def test_arena_names_the_buffer_behind_a_store_past_its_end():
    A = _arena()
    A.mem[A.bufs["out"].end] = 0
    with pytest.raises(ArenaError) as e:
        A.check("one byte past")
    msg = str(e.value)
    assert "0 bytes PAST the end of 'out'" in msg and "offset +84 from the buffer's start, +0 from its end" in msg
    assert "found [5a 5a 5a 5a 00 a5" in msg and "expected [5a 5a 5a 5a a5 a5" in msg


def test_arena_names_the_buffer_behind_a_store_before_its_start():
    A = _arena()
    A.mem[A.bufs["ws"].start - 1] = 7
    with pytest.raises(ArenaError) as e:
        A.check("one byte before")
    assert "1 bytes BEFORE the start of 'ws'" in str(e.value) and "offset -1 from the buffer's start" in str(e.value)


def test_arena_reports_a_changed_input_and_a_frozen_output():
    A = _arena()
    A.mem[A.bufs["xyz"].start + 20] ^= 1
    with pytest.raises(ArenaError) as e:
        A.check("input")
    assert "inside 'xyz' (role in" in str(e.value) and "offset +20 from the buffer's start" in str(e.value)
    A = _arena()
    A.view("out").fill_(2.0)
    A.freeze("out")  # from here on an input of later calls
    A.check("unchanged")
    A.view("out")[0, 0] = 3.0
    with pytest.raises(ArenaError, match="inside 'out'"):
        A.check("handle modified")


# ---- coverage: every entry point that takes a pointer has a contract case -------------------------------------------
EXCLUDED = {
    "rf_version": "no arguments: returns a static string",
    "rf_status_string": "no device tensors: maps a status to a static string",
    "rf_device_check": "no arguments: launches nothing",
    "rf_*_workspace_bytes": "host arithmetic on sizes: launches nothing",
    "rf_*_supported": "host arithmetic on sizes: launches nothing",
    "rf_profile_*": "host-side measurement hooks: host pointers only",
    "rf_probe_memset_async": "the diagnostic hipMemsetAsync (rf_probe_*): no kernel of the library",
}


def _takes_pointer(argtypes):
    return any(t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes)


def test_every_pointer_taking_entry_has_a_contract_case():
    from rfnet_amd._lib import SIGNATURES
    import test_gpu_memory_contract as T
    covered = set()
    for cid, (entries, fn) in T.CASES.items():
        assert entries and callable(fn), cid
        unknown = [e for e in entries if e not in SIGNATURES]
        assert not unknown, f"case {cid} names {unknown}, which include/rfops.h does not declare"
        covered.update(entries)
    missing = []
    for name, (_, argtypes) in SIGNATURES.items():
        if not _takes_pointer(argtypes) or name in covered:
            continue
        if not any(fnmatch.fnmatchcase(name, pat) for pat in EXCLUDED):
            missing.append(name)
    assert not missing, f"ABI entries without a memory-contract case (tests/test_gpu_memory_contract.py): {missing}"
    for pat, reason in EXCLUDED.items():
        assert reason and any(fnmatch.fnmatchcase(n, pat) for n in SIGNATURES), f"stale exclusion {pat}"
        # an exclusion may not hide an entry that takes device tensors: only the allowed families
        assert pat in ("rf_version", "rf_status_string", "rf_device_check") or pat.startswith("rf_profile_") \
            or pat.startswith("rf_probe_") or pat.endswith("_workspace_bytes") or pat.endswith("_supported")
    hidden = [n for n in covered if any(fnmatch.fnmatchcase(n, pat) for pat in EXCLUDED)]
    assert not hidden, f"both covered and excluded: {hidden}"
