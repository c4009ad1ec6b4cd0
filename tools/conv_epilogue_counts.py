#!/usr/bin/env python3
"""Wait and branch counts of the fused convolution's epilogue, from the compiler's assembly ("Epilogue: full tiles").

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Icsrc --cuda-device-only -S csrc/conv_x6.hip -o conv_x6.s
    python tools/conv_epilogue_counts.py conv_x6.s [--json FILE]

Per conv_split_kernel instantiation, over the EPILOGUE (everything behind the kernel's last MFMA):
    stores      16-byte global stores (tile stores and statistics records)
    masked      exec-masked blocks (s_and_saveexec)
    vm0         s_waitcnt with vmcnt(0)
    runs        the straight-line runs of 16-byte stores -- a run ends at a label or a branch -- as stores x runs, and `run_vm0`, the
                vmcnt(0) waits strictly between the first and the last store of any run of more than two stores (a tile quarter's eight
                stores; the two record stores are a run of two)
    loads       16-byte global loads (residual requests), and `load_runs`, their straight-line runs likewise
    full        the full-tile path: from the first store of the first run of more than two stores to the last store of the last such run
                (one contiguous piece of code: the quarters of the predicate-free epilogue) -- its vmcnt(0) waits / exec-masked blocks
                (the one around the two record stores of a quarter: lanes 0 .. 7 write them); "-" where there is no such path
It reads wait counts and branch counts only."""
import argparse
import json
import re
import sys
from collections import Counter

KERNEL = re.compile(r"^(_ZN5cddpm17conv_split_kernelILi(\d+)ELi(\d+)ELb([01])ELi(\d+)EEEvNS_8ConvArgsE):")
END = re.compile(r"^\.Lfunc_end\d+:")
LABEL = re.compile(r"^\.LBB\d+_\d+:")


def functions(lines):
    name, body = None, []
    for ln in lines:
        m = KERNEL.match(ln)
        if m:
            name, body = "<%s,%s,%s,%s>" % (m.group(2), m.group(3), "true" if m.group(4) == "1" else "false", m.group(5)), []
        elif name and END.match(ln):
            yield name, body
            name = None
        elif name:
            body.append(ln.strip())


def runs_of(body, opcode):
    """[(count, vmcnt(0) waits between the first and the last)] per straight-line run that holds the opcode"""
    out, n, waits, pending = [], 0, 0, 0
    for ins in body + [".LBB_end:"]:
        if LABEL.match(ins) or ins.startswith("s_cbranch") or ins.startswith("s_branch") or ins.startswith("s_endpgm"):
            if n:
                out.append((n, waits))
            n = waits = pending = 0
        elif ins.startswith(opcode):
            n += 1
            waits += pending
            pending = 0
        elif ins.startswith("s_waitcnt") and "vmcnt(0)" in ins and n:
            pending += 1
    return out


def full_span(ep):
    """(vmcnt(0) waits, exec-masked blocks) between the first and the last store of the runs of more than two stores, or None"""
    first = last = None
    start = n = 0
    for i, ins in enumerate(ep + [".LBB_end:"]):
        if LABEL.match(ins) or ins.startswith("s_cbranch") or ins.startswith("s_branch") or ins.startswith("s_endpgm"):
            if n > 2:
                first, last = (start if first is None else first), stop
            n = 0
        elif ins.startswith("global_store_dwordx4"):
            if n == 0:
                start = i
            n, stop = n + 1, i
    if first is None:
        return None
    span = ep[first:last + 1]
    return (sum(ins.startswith("s_waitcnt") and "vmcnt(0)" in ins for ins in span), sum(ins.startswith("s_and_saveexec") for ins in span))


def counts(body):
    last = max((i for i, ins in enumerate(body) if ins.startswith("v_mfma")), default=-1)
    ep = body[last + 1:]
    st, ld = runs_of(ep, "global_store_dwordx4"), runs_of(ep, "global_load_dwordx4")
    fmt = lambda rs: " ".join(f"{n}x{c}" for n, c in sorted(Counter(n for n, _ in rs).items(), reverse=True))
    return {"stores": sum(n for n, _ in st), "masked": sum(ins.startswith("s_and_saveexec") for ins in ep),
            "vm0": sum(ins.startswith("s_waitcnt") and "vmcnt(0)" in ins for ins in ep), "runs": fmt(st),
            "run_vm0": sum(w for n, w in st if n > 2), "full": full_span(ep), "loads": sum(n for n, _ in ld), "load_runs": fmt(ld)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("asm")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    with open(a.asm) as f:
        res = {name: counts(body) for name, body in functions(f.read().splitlines())}
    if not res:
        sys.exit("no conv_split_kernel in " + a.asm)
    print(f"{'kernel':18s} {'stores':>6s} {'masked':>6s} {'vm0':>4s} {'run_vm0':>7s}  {'runs':24s} {'loads':>5s}  {'load_runs':16s} full vm0/masked")
    for name, c in res.items():
        print(f"{name:18s} {c['stores']:6d} {c['masked']:6d} {c['vm0']:4d} {c['run_vm0']:7d}  {c['runs']:24s} {c['loads']:5d}  {c['load_runs']:16s} {'%d/%d' % tuple(c['full']) if c['full'] else '-'}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
