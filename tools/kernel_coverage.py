#!/usr/bin/env python3
"""Which GEMM (or, with --family attention / --family conv / --family embcnn, attention / convolution and pooling / emb_cnn data-path) kernels does a test run launch?  (tests/test_gpu_gemm_exact.py pins every arm of the
GEMM dispatch, tests/test_gpu_attention_arms.py every arm of the attention dispatch; this is the evidence.)

  tools/kernel_coverage.py asm OUT_DIR                 compile the device side of the GEMM translation units (csrc/gemm_nt.hip, gemm_nn.hip,
                                                       gemm_tn.hip, gemm_big.hip) to gfx950 assembly, as tools/isa_identity.py dump does for all
  tools/kernel_coverage.py report ASM_DIR ALL.csv [--auto AUTO.csv] [--wall NAME=SECONDS ...]
                                                       launches per GEMM kernel symbol (tools/isa_identity.py kernels() lists them per file) in
                                                       the kernel-trace CSV of
                                                         rocprofv3 --kernel-trace --stats -M -f csv -- python -m pytest tests/test_gpu_gemm_exact.py -q -m gpu
                                                       and, with --auto, in the trace of the same command with `-k auto` (the cases that set
                                                       no tuning hook); then the symbols never launched, and those launched only under a hook
                                                       with the dispatch line that keeps them from the automatic choice.  Exit status 1 if a
                                                       symbol was never launched.
  tools/kernel_coverage.py diff A.csv B.csv [--only REGEX]
                                                       the kernel names dispatched in kernel-trace A and never in B (names matched as `report`
                                                       matches them): A = a `bench.py --workload lowrank --steps 2 --warmup 1` run (bf16, and
                                                       again with --precision fp8), B = `pytest tests/test_gpu_lowrank_widths.py -m gpu` -- what the
                                                       benchmark step launches that the test file never does.  --only 'gemm|fp8' keeps the GEMM family.
                                                       Exit status 1 if the list is not empty.

The trace is matched by mangled name (rocprofv3 -M; a trailing .kd is dropped) or, for a demangled trace, by the c++filt form with white
space removed.  With `--family attention` both commands cover the five attention translation units that hold kernels (ATTENTION_FILES; csrc/attention.hip
holds the entry points and the dispatch, no kernel), and the trace is that
of tests/test_gpu_attention_arms.py (no tuning hook selects an attention kernel there: PARTS_ONLY lists the kernels that only a call with one
of ASR_ATTN_DQ / ASR_ATTN_DKV reaches).  With `--family conv` they cover the nine translation units of the convolution front end (CONV_FILES)
and the trace is that of tests/test_gpu_conv_arms.py; --auto is the trace of the same command with `-k "not hooked"` (the cases that set no
tuning hook carry no "hooked" in their ids), CONV_HOOK_ONLY explains the symbols only a hook reaches and CONV_HOOK_FORMS lists the launch
forms of a shared symbol that only a hook reaches.  Instantiations that exist only in -DASR_TUNE_ABLATE or C64_TIMING builds are not in a
default build's assembly and so not in the report.  With `--family embcnn` they cover csrc/embcnn.hip (im2col, col2im, window sum and
the BatchNorm kernels of the emb_cnn front end) and the trace is that of tests/test_gpu_embcnn_arms.py; no tuning hook selects a kernel of
that file.  With `--family decode` they cover csrc/decode.hip (the bf16 greedy step: asr_dec_gemm, asr_dec_attn, asr_dec_attn_fused,
asr_dec_finish) and the trace is that of tests/test_gpu_decode_arms.py; no tuning hook selects a kernel of that file.
`--group NAME=CSV` (any family, repeatable) adds a column with the launches in the trace of a part of the file -- the same command with
`-k NAME` -- so that the report says which cases reach which symbol.  The counter run is a run of its own: no --pmc next to the tracing."""
import argparse
import collections
import csv
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_identity  # noqa: E402

GEMM_FILES = ("gemm_nt.hip", "gemm_nn.hip", "gemm_tn.hip", "gemm_big.hip")
ATTENTION_FILES = ("attention_generic.hip", "attention_d64_fwd.hip", "attention_d64_bwd.hip", "attention_d64_bwd_fused.hip", "attention_pp.hip")
CONV_FILES = ("conv1.hip", "conv1_wgrad_mfma.hip", "conv_igemm.hip", "conv_c64.hip", "conv_ws.hip", "conv_wgrad.hip", "conv_wgrad_dma.hip",
              "conv_level0.hip", "pool.hip")
EMBCNN_FILES = ("embcnn.hip",)
DECODE_FILES = ("decode.hip",)
FAMILIES = {"gemm": GEMM_FILES, "attention": ATTENTION_FILES, "conv": CONV_FILES, "embcnn": EMBCNN_FILES, "decode": DECODE_FILES}
LABEL = {"gemm": "GEMM", "attention": "attention", "conv": "convolution / pooling", "embcnn": "emb_cnn data-path", "decode": "decode-step"}

# kernels the automatic dispatch cannot choose: (substring of the demangled name, the line that decides)
HOOK_ONLY = (
    ("gemm_glds_kernel<float, float, 128, 128, 1>", "gemm_nt.hip dispatch_fast: 128 x 128 four-wave blocks only under GEMM_TILE = 0"),
    ("gemm_glds_kernel<unsigned short, unsigned short, 128, 128, 1>", "gemm_nt.hip dispatch_fast: 128 x 128 four-wave blocks only under GEMM_TILE = 0"),
    ("gemm_glds_kernel<unsigned short, float, 128, 128, 1>", "gemm_nt.hip dispatch_fast: 128 x 128 four-wave blocks only under GEMM_TILE = 0"),
    ("gemm_glds_kernel<unsigned short, float, 128, 64, 1>", "gemm_nt.hip dispatch_fast: 128 x 64 needs sizeof(TO) == sizeof(T); else GEMM_TILE = 1"),
    ("gemm_big_nt_kernel<256, 256, 2, unsigned short>", "gemm_big.hip asr_gemm_big_nt: 256 x 256 blocks for fp32 output only; bf16 under GEMM_BIG = 256"),
    ("gemm_big_nt_kernel<128, 128, 3, unsigned short>", "gemm_big.hip asr_gemm_big_nt: ns is 2 or 4 unless GEMM_BIG_NS = 3"),
    ("gemm_big_nn_kernel<3>", "gemm_big.hip asr_gemm_big_nn: ns is 2 or 4 unless GEMM_BIG_NS = 3"),
    ("gemm_tn128g_kernel<3>", "gemm_tn.hip asr_gemm_tn_grouped: 128 x 128 grouped blocks only under TN_GROUP_TILE = 128"),
)

# convolution kernels the automatic dispatch cannot choose
_C64_WHY = "conv_c64.hip asr_conv3x3_c64_launch: 8-wave workgroups on %s tiles only under C64_SHAPE = %d (default 0: 8 x 16, two 4-wave workgroups per CU)"
CONV_HOOK_ONLY = (
    ("conv3x3_c64_kernel<16, 16, true, 3, false>", _C64_WHY % ("16 x 16", 1)),
    ("conv3x3_c64_kernel<16, 16, false, 3, false>", _C64_WHY % ("16 x 16", 1)),
    ("conv3x3_c64_kernel<32, 8, true, 3, false>", _C64_WHY % ("8 x 32", 2)),
    ("conv3x3_c64_kernel<32, 8, false, 3, false>", _C64_WHY % ("8 x 32", 2)),
)
# launch forms of a symbol that other shapes reach without a hook: (form, the line that decides)
CONV_HOOK_FORMS = (
    ("conv3x3_c64_kernel<16, 8, false, 3, false> twice with ypix = 256 (64 -> 128 in two passes)",
     "conv_igemm.hip asr_conv3x3_igemm: bf16 64 -> 128 without a mask runs conv_ws.hip in one pass unless WS64 = 0"),
    ("conv3x3_igemm_kernel<bf16, 64 | 128, 16, 1, 1, false> with 128 input channels",
     "conv_igemm.hip asr_conv3x3_igemm: bf16 with Cin = 128 runs conv_ws.hip unless WS128 = 0 (Cin = 192 and 64 -> 128 with a mask reach the symbols)"),
    ("conv3x3_igemm_kernel<bf16, 128, 16, 1, 1, true> with 128 input channels (pooled epilogue)",
     "conv_igemm.hip conv3x3_relu_pool_tcf_code_impl: Cin = 128 runs conv_ws.hip unless WS128 = 0 (Cin = 64 reaches the symbol)"),
    ("conv3x3_ws128_kernel<128, 8, 128, 0, 1> at H % 16 == 0 (single tiles)",
     "conv_ws.hip asr_conv3x3_ws128_launch: vertical tile pairs at H % 16 == 0 unless WS_PAIR = 0 (H % 16 == 8 reaches the symbol)"),
    ("vgg_level0_fwd / _dgrad / _wgrad_kernel with wsplit = 0",
     "conv_level0.hip: conv.0 on split weights unless L0_WSPLIT = 0 (an argument of the same kernels)"),
)
HOOK_ONLY_OF = {"gemm": HOOK_ONLY, "attention": (), "conv": CONV_HOOK_ONLY, "embcnn": (), "decode": ()}

# attention kernels that ops.attn_bwd never chooses (it asks for dQ and dK / dV in one launch): reached by a direct asr_attn_bwd call with one part
PARTS_ONLY = (
    ("attn_bwd_dq_bf16_d64_kernel<1>", "attention.hip attn_choose_bwd: dQ alone (attention_d64_bwd.hip) only when parts has ASR_ATTN_DQ without ASR_ATTN_DKV"),
    ("attn_bwd_dkv_bf16_d64_kernel<1>", "attention.hip attn_choose_bwd: dK / dV alone (attention_d64_bwd.hip) only when parts has ASR_ATTN_DKV without ASR_ATTN_DQ"),
)


def dump_asm(out, files=GEMM_FILES):
    b = isa_identity._build_module(isa_identity.ROOT)
    os.makedirs(out, exist_ok=True)
    flags = [f for f in b.FLAGS if f != "-fPIC"]
    for name in files:
        cmd = [b._hipcc()] + flags + b.PER_FILE_FLAGS.get(name, []) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, name), "-o",
                                                                      os.path.join(out, name + ".s")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (name, r.stderr[-4000:]))
        print("assembled", name, flush=True)


def family_kernels(asm_dir, files=GEMM_FILES):
    """[(file, mangled symbol)] of every __global__ kernel of the family's translation units (a symbol with an .amdhsa block)."""
    out = []
    for f in files:
        ks = isa_identity.kernels(os.path.join(asm_dir, f + ".s"))
        out += [(f, s) for s in sorted(ks) if ks[s][1] is not None]
    return out


def demangle(symbols):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True)
        names = r.stdout.split("\n")[:len(symbols)]
        if r.returncode == 0 and len(names) == len(symbols):
            return dict(zip(symbols, names))
    except OSError:
        pass
    return {s: s for s in symbols}


def _key(name):
    """What a kernel name is matched by: no `.kd` / clone suffix, no return type, no white space."""
    name = re.sub(r"\s*\[clone [^\]]*\]$", "", name.strip())
    name = re.sub(r"\.kd$", "", name)
    if name.startswith("void "):
        name = name[5:]
    return re.sub(r"\s+", "", name)


def launch_counts(lines):
    """{matching key of a kernel name: dispatches} from the lines of a rocprofv3 kernel-trace CSV (an open file or a list of lines)."""
    counts = collections.Counter()
    for row in csv.DictReader(lines):
        name = row.get("Kernel_Name") or row.get("KernelName") or row.get("Name")
        if name:
            counts[_key(name)] += 1
    return counts


def coverage(symbols, names, counts):
    """{symbol: dispatches}: a symbol is counted under its mangled name and under its demangled one."""
    out = {}
    for s in symbols:
        keys = {_key(s), _key(names.get(s, s))}
        out[s] = sum(counts.get(k, 0) for k in keys)
    return out


def report(asm_dir, all_csv, auto_csv, walls, family="gemm", groups=()):
    ks = family_kernels(asm_dir, FAMILIES[family])
    syms = [s for _, s in ks]
    names = demangle(syms)
    with open(all_csv, newline="") as fh:
        call = coverage(syms, names, launch_counts(fh))
    cauto = None
    if auto_csv:
        with open(auto_csv, newline="") as fh:
            cauto = coverage(syms, names, launch_counts(fh))
    cgroup = []
    for g in groups:
        gname, gcsv = g.split("=", 1)
        with open(gcsv, newline="") as fh:
            cgroup.append((gname, coverage(syms, names, launch_counts(fh))))
    for w in walls:
        print("wall time  %s s" % w.replace("=", "  "))
    gcols = "".join(" %11s" % n[:11] for n, _ in cgroup)
    print("%-18s %9s %9s%s  kernel" % ("file", "launches", "no hook" if cauto is not None else "", gcols))
    for f, s in ks:
        print("%-18s %9d %9s%s  %s" % (f, call[s], cauto[s] if cauto is not None else "", "".join(" %11d" % c[s] for _, c in cgroup), names[s]))
    never = [s for s in syms if call[s] == 0]
    print("\n%s kernel symbols: %d, launched: %d, never launched: %d" % (LABEL[family], len(syms), len(syms) - len(never), len(never)))
    for s in never:
        print("  NEVER  %s" % names[s])
    if family == "attention":
        for sub, why in PARTS_ONLY:
            for s in syms:
                if sub in names[s]:
                    print("  PARTS  %s: %d launches\n         %s" % (names[s], call[s], why))
    if cauto is not None:
        hook = [s for s in syms if call[s] > 0 and cauto[s] == 0]
        print("launched only with a tuning hook set: %d" % len(hook))
        for s in hook:
            why = [w for sub, w in HOOK_ONLY_OF[family] if sub in names[s]]
            print("  HOOK   %s\n         %s" % (names[s], why[0] if why else "NOT EXPLAINED: a case without a hook should reach it"))
    if family == "conv":
        print("launch forms of a shared symbol that only a tuning hook reaches: %d" % len(CONV_HOOK_FORMS))
        for form, why in CONV_HOOK_FORMS:
            print("  FORM   %s\n         %s" % (form, why))
    return 1 if never else 0


def diff(a_csv, b_csv, only=None):
    """Kernel names (matched as `report` matches them: launch_counts' keys) dispatched in kernel-trace A and never in B, with their
    dispatches in A; `only`: a regular expression the c++filt form of the name must contain.  Exit status 1 if there is one."""
    with open(a_csv, newline="") as fh:
        ca = launch_counts(fh)
    with open(b_csv, newline="") as fh:
        cb = launch_counts(fh)
    na, nb = demangle(sorted(ca)), demangle(sorted(cb))                    # key -> c++filt form (a demangled key stays itself)
    have = set(cb) | {_key(v) for v in nb.values()}                        # a mangled name in one trace may be demangled in the other
    missing = []
    for k in sorted(ca):
        if k in have or _key(na[k]) in have:
            continue
        if only and not re.search(only, na[k]):
            continue
        missing.append((na[k], ca[k]))
    print("kernel names dispatched in %s: %d, in %s: %d%s" % (a_csv, len(ca), b_csv, len(cb), ", filter %r" % only if only else ""))
    print("dispatched in the first trace and never in the second: %d" % len(missing))
    for shown, n in missing:
        print("  ONLY-A %9d  %s" % (n, shown))
    return 1 if missing else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    a_ = sub.add_parser("asm")
    a_.add_argument("out")
    a_.add_argument("--family", choices=sorted(FAMILIES), default="gemm")
    r_ = sub.add_parser("report")
    r_.add_argument("asm_dir")
    r_.add_argument("all_csv")
    r_.add_argument("--auto")
    r_.add_argument("--wall", action="append", default=[])
    r_.add_argument("--family", choices=sorted(FAMILIES), default="gemm")
    r_.add_argument("--group", action="append", default=[], metavar="NAME=CSV")
    d_ = sub.add_parser("diff")
    d_.add_argument("a_csv")
    d_.add_argument("b_csv")
    d_.add_argument("--only", metavar="REGEX")
    a = ap.parse_args()
    if a.cmd == "asm":
        dump_asm(a.out, FAMILIES[a.family])
    elif a.cmd == "diff":
        sys.exit(diff(a.a_csv, a.b_csv, a.only))
    else:
        sys.exit(report(a.asm_dir, a.all_csv, a.auto, a.wall, a.family, a.group))
