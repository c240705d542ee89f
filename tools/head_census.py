#!/usr/bin/env python3
"""Static census of what lmpc_solve_group runs outside its round loop, from the compiler's assembly (hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC
-I../../include --cuda-device-only -S lmpc_fast.hip): the kernel's body cut at its workgroup barriers and at the round loop (the longest backward branch, as
profiles/r09_round_isa_census.txt found it), and per piece the instructions that move values between lanes -- ds_bpermute_b32 (the LDS crossbar), DPP moves,
gfx950's lane swaps, v_readlane -- the MFMAs and the LDS instructions.  Pieces are in the order of the text, which is the order of execution for the head
(straight-line code between barriers); the piece behind the loop holds the finish and every cold path the compiler placed there.
    python tools/head_census.py fast_parent.s fast_change.s ['lmpc_solve_group<1, 1>']"""
import re, subprocess, sys

KINDS = [("ds_bpermute_b32", r"^ds_bpermute_b32"), ("DPP moves (v_mov_b32_dpp)", r"^v_mov_b32_dpp"), ("v_permlane32_swap_b32", r"^v_permlane32_swap"),
         ("v_permlane16_swap_b32", r"^v_permlane16_swap"), ("v_readlane_b32", r"^v_readlane_b32"), ("v_mfma_f64_16x16x4", r"^v_mfma_f64_16x16x4"),
         ("v_add_f64", r"^v_add_f64"), ("LDS instructions (ds_*)", r"^ds_"), ("s_waitcnt", r"^s_waitcnt"), ("instructions (all)", r"^[a-z]")]


def body(path, want):
    txt = open(path).read()
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if name.startswith("void mpcx::(anonymous namespace)::" + want) or name.startswith(want):
            return [l.strip() for l in m.group(2).splitlines() if l.strip() and not l.strip().startswith(";")]
    raise SystemExit("kernel %s not found in %s" % (want, path))


def pieces(lines):
    label = {l[:-1]: i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:$", l)}
    best = (0, 0, 0)
    for i, l in enumerate(lines):
        m = re.match(r"^s_c?branch\w*\s+(?:\w+,\s*)?(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label and label[m.group(1)] < i and i - label[m.group(1)] > best[0]:
            best = (i - label[m.group(1)], label[m.group(1)], i)
    lo, hi = best[1], best[2]
    bars = [i for i, l in enumerate(lines) if l.startswith("s_barrier") and i < lo]
    cuts = [0] + [b + 1 for b in bars] + [lo, hi + 1, len(lines)]
    names = ["entry .. barrier 1 (staging)"] + ["barrier %d .. barrier %d" % (k, k + 1) for k in range(1, len(bars))] + ["barrier %d .. round loop" % len(bars), "round loop", "behind the round loop (finish)"]
    return [(n, lines[a:b]) for n, a, b in zip(names, cuts[:-1], cuts[1:])]


def main():
    want = sys.argv[3] if len(sys.argv) > 3 else "lmpc_solve_group<1, 1>"
    cols = [pieces(body(p, want)) for p in sys.argv[1:3]]
    print("%s: %s | %s" % (want, sys.argv[1], sys.argv[2]))
    for k in range(max(len(c) for c in cols)):
        print("\n%s" % " | ".join(c[k][0] if k < len(c) else "-" for c in cols))
        for kind, rx in KINDS:
            n = [sum(1 for l in c[k][1] if re.match(rx, l)) if k < len(c) else 0 for c in cols]
            print("  %-28s %6d %6d" % (kind, n[0], n[1]))
    print("\nwhole kernel")
    for kind, rx in KINDS:
        n = [sum(1 for _, ls in c for l in ls if re.match(rx, l)) for c in cols]
        print("  %-28s %6d %6d" % (kind, n[0], n[1]))


if __name__ == "__main__":
    main()
