#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel: `tools/isa_diff.py DIR_A DIR_B [-DFLAG ...] [--only FILE ...]`.

Every decode source and every source of build.STAGE_SOURCES (the MLA prefill forward and backward among them) of each tree (DIR = a checkout of this
repository) is compiled to assembly with the flags of the build, the assembly is cut
into kernels (symbol to .Lfunc_end, plus the .amdhsa_kernel descriptor block), comments are stripped and local labels renumbered, and the texts are
compared.  Reports the kernels that exist on one side only and those whose text differs; exit status 1 on any difference.  The aid of a refactor
that promises "no kernel's instructions change".  Flags after the directories (-D...) go to both compiles: the experiment switches."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flash-attention-turing_amd"))
import build  # noqa: E402

DECODE_SOURCES = [s for s in build.HIP_SOURCES if "kvcache" in s or s in build.STAGE_SOURCES]      # the decode sources and every staged 64-row body


def kernels(tree, source, flags):
    """{kernel symbol: normalised text} of one source file of `tree`"""
    csrc = os.path.join(tree, "flash-attention-turing_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        cmd = [build.hipcc_path()] + build.HIPCC_FLAGS + build.EXTRA_FLAGS.get(source, []) + flags + ["-I", csrc, "-I", os.path.join(tree, "include"),
                                                                                                    "--cuda-device-only", "-S", os.path.join(csrc, source), "-o", asm]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{tree}: {source}: hipcc failed\n{r.stderr[-2000:]}")
        txt = open(asm).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel", txt, re.M | re.S):
        name = m.group(1)
        body = txt[txt.index("\n" + name + ":"):]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()] + m.group(0)
        body = re.sub(r";.*", "", body)                                     # comments
        labels = {}
        body = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), body)
        out[name] = "\n".join(x.strip() for x in body.splitlines() if x.strip())
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("--only", nargs="+", default=DECODE_SOURCES, metavar="FILE", help="sources to compare (default: every decode source)")
    a, flags = ap.parse_known_args()
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        jobs = [(s, ex.submit(kernels, a.dir_a, s, flags), ex.submit(kernels, a.dir_b, s, flags)) for s in a.only]
        bad = 0
        for s, fa, fb in jobs:
            ka, kb = fa.result(), fb.result()
            only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
            differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
            print(f"{s}: {len(ka)} / {len(kb)} kernels, {len(only_a)} only in A, {len(only_b)} only in B, {len(differ)} differ")
            for tag, names in (("only in A", only_a), ("only in B", only_b), ("differs", differ)):
                for k in names:
                    print(f"  {tag}: {k}")
            bad += len(only_a) + len(only_b) + len(differ)
    print(f"{' '.join(flags) or '(no flag)'}: {bad} difference(s)")
    sys.exit(1 if bad else 0)
