"""Static instruction counts of nnp_sort_reg_kernel per stamped phase, from the compiler's assembly:
    hipcc <the flags of rfnet_amd/build.py> --cuda-device-only -S rfnet_amd/csrc/nn_pruned.hip -o nn_pruned.s
    python tools/experiments/sort_phase_counts.py nn_pruned.s [mangled-name substring, default ILb0ELb0E or ILb0E]
A phase is the text between two reads of the shader clock (the `stamp()` calls); the text order of the assembly is the
program order here because the kernel's phases are separated by barriers.  The staging round's loops are rolled (`unroll 1`
outside, 4 inside), so their counts are per trip, not per thread.  Counts are static: an instruction under a branch counts once."""
import collections
import re
import sys

PHASES = ["prologue", "loads issued+zeroed", "bbox+tables", "quantiles", "keys+hist", "scan", "positions",
          "staging: scatter", "staging: boxes", "staging: write-out", "epilogue"]


def kernel_body(text, want):
    names = [m.group(1) for m in re.finditer(r"^(_ZN\S*nnp_sort_reg_kernel\S*):", text, re.M)]
    name = [n for n in names if want in n][0]
    body = text.split("\n" + name + ":", 1)[1].split(".Lfunc_end", 1)[0]
    return name, body.splitlines()


def klass(op):
    if op.startswith(("v_", "V_")):
        return "VALU"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "other"


def main():
    text = open(sys.argv[1]).read()
    want = sys.argv[2] if len(sys.argv) > 2 else ("ILb0ELb0E" if "nnp_sort_reg_kernelILb0ELb0E" in text else "ILb0E")
    name, lines = kernel_body(text, want)
    phase = 0
    per = [collections.Counter() for _ in PHASES]
    ops = [collections.Counter() for _ in PHASES]
    for ln in lines:
        ln = ln.split(";", 1)[0].strip()
        if not ln or ln.startswith(".") or ln.endswith(":"):
            continue
        tok = ln.split()
        op = tok[0]
        if op in ("s_memtime", "s_memrealtime"):
            phase = min(phase + 1, len(PHASES) - 1)
            continue
        if op in ("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_branch") or op.startswith("s_cbranch"):
            per[phase]["wait/branch"] += 1
            continue
        per[phase][klass(op)] += 1
        key = op
        # a canonicalisation: both sources the same register (the destination may be another one)
        if op in ("v_max_f32_e32", "v_max_f32_e64", "v_max_f32") and len(tok) == 4 and tok[2].rstrip(",") == tok[3].rstrip(","):
            key = "v_max_f32 x,x,x"
        ops[phase][key] += 1
    print(name)
    print(f"{'phase':22s} {'VALU':>6s} {'SALU':>6s} {'LDS':>5s} {'VMEM':>5s}   canon  v_mov  med3 cvt_i32 cvt_pk_u8  and  min/max")
    tot = collections.Counter()
    allops = collections.Counter()
    for i, p in enumerate(PHASES):
        o = ops[i]
        mm = sum(v for k, v in o.items() if re.match(r"v_(min|max)3?_f32", k))
        print(f"{p:22s} {per[i]['VALU']:6d} {per[i]['SALU']:6d} {per[i]['LDS']:5d} {per[i]['VMEM']:5d}   "
              f"{o['v_max_f32 x,x,x']:5d} {sum(v for k, v in o.items() if k.startswith('v_mov_b32')):6d} "
              f"{sum(v for k, v in o.items() if k.startswith('v_med3_f32')):5d} {sum(v for k, v in o.items() if k.startswith('v_cvt_i32_f32')):7d} "
              f"{sum(v for k, v in o.items() if k.startswith('v_cvt_pk_u8_f32')):9d} {sum(v for k, v in o.items() if k.startswith('v_and_b32')):4d} {mm:8d}")
        tot.update(per[i])
        allops.update(o)
    print(f"{'kernel':22s} {tot['VALU']:6d} {tot['SALU']:6d} {tot['LDS']:5d} {tot['VMEM']:5d}   {allops['v_max_f32 x,x,x']:5d} "
          f"{sum(v for k, v in allops.items() if k.startswith('v_mov_b32')):6d}")
    if len(sys.argv) > 3:
        i = PHASES.index(sys.argv[3])
        for k, v in ops[i].most_common(40):
            print(f"    {k:28s} {v}")


if __name__ == "__main__":
    main()
