#!/usr/bin/env python3
"""Proves that a host-side refactor left the device code alone.

  tools/isa_identity.py dump OUT_DIR [--tree TREE]    compile the device side of every csrc/*.hip of TREE (default: this tree) to
                                                      gfx950 assembly with the flags of asr_hip/build.py (as tests/test_isa_static.py does)
  tools/isa_identity.py compare BEFORE_DIR AFTER_DIR  per file: kernels before / after, the names removed, and how many surviving kernels
                                                      differ in instruction text or in their .amdhsa_* block (exit status 1 if any does,
                                                      or if AFTER has a kernel BEFORE has not)
  tools/isa_identity.py compare --by-symbol BEFORE_DIR AFTER_DIR
                                                      the same comparison over the union of the symbols of all files of each dump, for a
                                                      change that moves kernels between files (same normalisation, same exit status rule,
                                                      a symbol whose copies in two files of AFTER differ from each other counts as
                                                      differing, and so does a kernel that AFTER defines in two files unless BEFORE has
                                                      it in two files too, with identical copies: a kernel shared through a header, as
                                                      ctc_lse_kernel of ctc_common.h)

Kernels are split at their `_Z...:` labels.  The function index in local labels (.LBB<n>_<m>, .Lfunc_end<n>, ...) shifts when a
neighbour is deleted, so it is normalised before the comparison.  hipcc gives a kernel in an anonymous namespace the same name
(_ZN12_GLOBAL__N_1...) whatever file it is compiled in -- no per-file suffix is appended without -fgpu-rdc -- so --by-symbol matches
the names as they are.  A __device__ variable in a header (a zero page) is a symbol of every file that uses it; identical copies are
one symbol."""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "end2end-asr-pytorch_amd"


def _build_module(tree):
    spec = importlib.util.spec_from_file_location("_asr_build", os.path.join(tree, PKG, "asr_hip", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def dump(tree, out):
    b = _build_module(tree)
    os.makedirs(out, exist_ok=True)
    hipcc = b._hipcc()
    flags = [f for f in b.FLAGS if f != "-fPIC"]

    def one(name):
        cmd = [hipcc] + flags + b.PER_FILE_FLAGS.get(name, []) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, name), "-o",
                                                                 os.path.join(out, name + ".s")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (name, r.stderr[-4000:]))
        print("assembled", name, flush=True)

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(one, sorted(f for f in os.listdir(b.CSRC) if f.endswith(".hip"))))


_LOCAL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")


def _norm(line):
    line = line.split(";")[0].rstrip()                     # comments carry source line numbers
    return _LOCAL.sub(lambda m: ".L%sN%s" % (m.group(1), m.group(3) or ""), line)


def kernels(path):
    """{symbol: (instruction text, .amdhsa block)} of one assembly file."""
    lines = open(path).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
    text = {}
    for n, a in enumerate(starts):
        sym = lines[a].split(":")[0]
        end = starts[n + 1] if n + 1 < len(starts) else len(lines)
        body = []
        for l in lines[a + 1:end]:
            if l.startswith("\t.section") or l.startswith("\t.rodata") or l.startswith("\t.amdgpu_metadata"):
                break                                      # the kernel descriptor / metadata that follow the code
            t = _norm(l).strip()
            if not t or t.startswith(".") and not t.endswith(":"):
                continue                                   # directives (.p2align, .loc, .size ...): not instructions
            body.append(t)
        text[sym] = body
    hsa, cur = {}, None
    for l in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)
            hsa[cur] = []
        elif cur is not None:
            if l.strip() == ".end_amdhsa_kernel":
                cur = None
            else:
                hsa[cur].append(_norm(l).strip())
    return {s: (text[s], hsa.get(s)) for s in text}         # a device function that was not inlined has no .amdhsa block: None


def compare(before, after):
    bad = 0
    tb = ta = 0
    for f in sorted(os.listdir(before)):
        if not f.endswith(".s"):
            continue
        kb, ka = kernels(os.path.join(before, f)), kernels(os.path.join(after, f))
        removed, added = sorted(set(kb) - set(ka)), sorted(set(ka) - set(kb))
        differ = [s for s in sorted(set(ka) & set(kb)) if ka[s] != kb[s]]
        tb, ta = tb + len(kb), ta + len(ka)
        print("%s: kernels %d -> %d, removed %d, added %d, %d differing" % (f[:-2], len(kb), len(ka), len(removed), len(added), len(differ)))
        for s in removed:
            print("  removed  %s" % _demangle(s))
        for s in added:
            print("  ADDED    %s" % _demangle(s))
        for s in differ:
            what = [w for w, i in (("text", 0), ("amdhsa", 1)) if ka[s][i] != kb[s][i]]
            print("  DIFFERS  %s (%s)" % (_demangle(s), ", ".join(what)))
        bad += len(added) + len(differ)
    print("total: kernels %d -> %d, %d added or differing" % (tb, ta, bad))
    return 1 if bad else 0


def _union(d):
    """({symbol: (text, amdhsa)} over all files of a dump, the symbols whose copies in two files differ, the kernels that two files define
    with identical copies)."""
    all_, diverging, shared = {}, set(), set()
    for f in sorted(os.listdir(d)):
        if not f.endswith(".s"):
            continue
        for s, v in kernels(os.path.join(d, f)).items():
            if s in all_ and all_[s] != v:
                diverging.add(s)
            elif s in all_ and v[1] is not None:
                shared.add(s)
            all_.setdefault(s, v)
    return all_, diverging, shared - diverging


def compare_by_symbol(before, after):
    (kb, _, shared_before), (ka, diverging, shared) = _union(before), _union(after)
    twice = diverging | (shared - shared_before)
    removed, added = sorted(set(kb) - set(ka)), sorted(set(ka) - set(kb))
    differ = [s for s in sorted(set(ka) & set(kb)) if ka[s] != kb[s] or s in twice]
    for s in removed:
        print("  removed  %s" % _demangle(s))
    for s in added:
        print("  ADDED    %s" % _demangle(s))
    for s in differ:
        what = [w for w, i in (("text", 0), ("amdhsa", 1)) if ka[s][i] != kb[s][i]] + (["defined in two files"] if s in twice else [])
        print("  DIFFERS  %s (%s)" % (_demangle(s), ", ".join(what)))
    nk = lambda k: sum(1 for v in k.values() if v[1] is not None)
    print("all files: symbols %d -> %d (kernels %d -> %d), removed %d, added %d, %d differing" %
          (len(kb), len(ka), nk(kb), nk(ka), len(removed), len(added), len(differ)))
    return 1 if added or differ else 0


def _demangle(sym):
    try:
        r = subprocess.run(["c++filt", sym], capture_output=True, text=True)
        return r.stdout.strip() or sym
    except OSError:
        return sym


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--tree", default=ROOT)
    c = sub.add_parser("compare")
    c.add_argument("--by-symbol", action="store_true")
    c.add_argument("before")
    c.add_argument("after")
    a = ap.parse_args()
    if a.cmd == "dump":
        dump(os.path.abspath(a.tree), a.out)
    else:
        sys.exit((compare_by_symbol if a.by_symbol else compare)(a.before, a.after))
