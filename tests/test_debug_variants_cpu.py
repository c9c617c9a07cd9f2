"""CPU: the adversarial-timing builds of flash-attention-turing_amd/build.py (DEBUG_VARIANTS) are what they say they are.

tests/test_dma_protocol_gpu.py and tests/test_stage_protocol_gpu.py ask those builds for the product's bits.  A mistyped -D builds the product again and
every such comparison passes - vacuously.  Here every (variant, rebuilt source) pair is compiled to gfx950 assembly with the line the build uses (the
file's EXTRA_FLAGS included; hipcc cross-compiles without a GPU) and compared with the product's assembly of the same source:
  * it builds, and its text differs from the product's;
  * the sleepy / slow builds contain more s_sleep than the product (which has none), and the same LDS-DMA statements;
  * the late-issue builds MOVE their LDS-DMA statements and do not drop them.  Counted per file as `buffer_load_dwordx4 .. lds`:
      fa_fwd_pp.hip                      one request site per site of the product: the same number as the product;
      fa_bwd.hip, fa_bwd_dq16.hip,       the product holds every loop request twice, once for the waves that issue at the top of the tile and once for
      fa_bwd_dkdv16.hip                  the staggered waves 4-7, the late form once for all eight: the same number as the product built WITHOUT the stagger
                                         (FA_DQ_STAGGER_DMA=0 FA_KV_STAGGER_DMA=0 / FA_DQ16_STAGGER_DMA=0 / FA_KV16_DMA_EARLY=2), and fewer than the product;
      fa_fwd_pp16.hip                    its late form (round 5) is another loop: it requests tile u + 1 where the counted wait of the product retires it
                                         and tile u + 2 is requested - at least the product's number, nothing dropped;
  * every macro a variant sets occurs in every source it rebuilds (the source and the project headers it includes, but for the header of the defaults);
  * the step of the staged bodies, with its racy form, is written in one file (fa_kvcache_stage.hpp);
  * no build of a decode kernel acquires scratch or another LDS size (the launch shape is the product's)."""
import concurrent.futures
import os
import re
import subprocess
import tempfile

import pytest

import _kernel_isa

fa_build = _kernel_isa._build

UNSTAGGERED = {"fa_bwd.hip": ["-DFA_DQ_STAGGER_DMA=0", "-DFA_KV_STAGGER_DMA=0"], "fa_bwd_dq16.hip": ["-DFA_DQ16_STAGGER_DMA=0"], "fa_bwd_dkdv16.hip": ["-DFA_KV16_DMA_EARLY=2"]}
PAIRS = [(n, s) for n, v in fa_build.DEBUG_VARIANTS.items() for s in v]
SLEEPING = [(n, s) for n, s in PAIRS if n in ("dma_sleepy", "stage_slow_reader", "stage_slow_writer", "stage_racy_slow_writer")]
LATE = [(n, s) for n, s in PAIRS if n == "dma_late"]
STAGE = [(n, s) for n, s in PAIRS if s in fa_build.STAGE_SOURCES]


def _lds_dma(text):
    return len(re.findall(r"buffer_load_dwordx4 [^\n]* lds", text))


def _resources(text):
    """{kernel: (scratch bytes a lane, LDS bytes a workgroup)} from the kernels' metadata"""
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        f = {k: int(v) for k, v in re.findall(r"\.amdhsa_(group_segment_fixed_size|private_segment_fixed_size) (\d+)", m.group(2))}
        out[m.group(1)] = (f["private_segment_fixed_size"], f["group_segment_fixed_size"])
    return out


@pytest.fixture(scope="module")
def asm():
    """{(variant or "product" or "unstaggered", source): assembly text or the compiler's error}: every build once, as many compilers at a time as cores (at most 16)"""
    jobs = {("product", s): [] for s in sorted({s for _, s in PAIRS})}
    jobs.update({("unstaggered", s): f for s, f in UNSTAGGERED.items()})
    jobs.update({(n, s): fa_build.DEBUG_VARIANTS[n][s] for n, s in PAIRS})
    with tempfile.TemporaryDirectory() as td:
        def run(item):
            (name, src), flags = item
            out = os.path.join(td, f"{name}__{src[:-4]}.s")
            r = subprocess.run(fa_build.debug_compile_command(src, flags, out, assembly=True), capture_output=True, text=True)
            if r.returncode != 0:
                return (name, src), RuntimeError(r.stderr[-2000:])
            with open(out) as f:
                return (name, src), f.read()

        with concurrent.futures.ThreadPoolExecutor(max(1, min(os.cpu_count() or 1, 16))) as ex:
            return dict(ex.map(run, jobs.items()))


def _text(asm, name, src):
    t = asm[(name, src)]
    assert isinstance(t, str), f"{name} / {src} does not build: {t}"
    return t


@pytest.mark.parametrize("name,src", PAIRS, ids=[f"{n}-{s[:-4]}" for n, s in PAIRS])
def test_variant_builds_and_is_not_the_product(asm, name, src):
    got, product = _text(asm, name, src), _text(asm, "product", src)
    assert "v_mfma" in got and got != product, f"{name} / {src}: the switches {fa_build.DEBUG_VARIANTS[name][src]} change nothing - the GPU comparison would be vacuous"


def _source_text(src, seen=None):
    """the text of a source of csrc/ with the project headers it includes by `#include "..."`, transitively; not fa_kvcache_stage_debug.hpp, which only
    defines the defaults of the stage macros and would make every source that includes it know them"""
    seen = set() if seen is None else seen
    path = os.path.join(fa_build.CSRC, src)
    if src in seen or src == "fa_kvcache_stage_debug.hpp" or not os.path.exists(path):
        return ""
    seen.add(src)
    with open(path) as f:
        text = f.read()
    return text + "".join(_source_text(h, seen) for h in re.findall(r'^\s*#include "([^"]+)"', text, re.M))


@pytest.mark.parametrize("name,src", PAIRS, ids=[f"{n}-{s[:-4]}" for n, s in PAIRS])
def test_every_macro_of_a_variant_occurs_in_the_source_it_rebuilds(name, src):
    text = _source_text(src)
    for flag in fa_build.DEBUG_VARIANTS[name][src]:
        m = re.fullmatch(r"-D(\w+)=\w+", flag)
        assert m, flag
        assert re.search(r"\b" + m.group(1) + r"\b", text), f"{name}: {src} does not know {m.group(1)}"


def _files(src, seen):
    """a source of csrc/ and the project headers it includes, transitively: {file name: text}"""
    path = os.path.join(fa_build.CSRC, src)
    if src in seen or not os.path.exists(path):
        return seen
    with open(path) as f:
        seen[src] = f.read()
    for h in re.findall(r'^\s*#include "([^"]+)"', seen[src], re.M):
        _files(h, seen)
    return seen


def test_the_stage_protocol_is_written_once():
    """The racy form is a preprocessor switch of the step, so a file with a preprocessor line that names FA_KVC_STAGE_RACY holds a copy of the step's
    protocol: over the staged sources and their headers that is fa_kvcache_stage.hpp alone, next to the header of the defaults."""
    files = {}
    for src in fa_build.STAGE_SOURCES:
        _files(src, files)
    assert all(s in files for s in fa_build.STAGE_SOURCES) and "fa_kvcache_stage_debug.hpp" in files
    holders = {name for name, text in files.items() if re.search(r"^[ \t]*#[^\n]*\bFA_KVC_STAGE_RACY\b", text, re.M)}
    assert holders == {"fa_kvcache_stage.hpp", "fa_kvcache_stage_debug.hpp"}, sorted(holders)


@pytest.mark.parametrize("name,src", SLEEPING, ids=[f"{n}-{s[:-4]}" for n, s in SLEEPING])
def test_sleeping_variants_sleep(asm, name, src):
    got, product = _text(asm, name, src), _text(asm, "product", src)
    assert product.count("s_sleep") == 0 and got.count("s_sleep") > 0
    assert _lds_dma(got) == _lds_dma(product)
    assert got.count("s_barrier") == product.count("s_barrier")


@pytest.mark.parametrize("name,src", LATE, ids=[f"{n}-{s[:-4]}" for n, s in LATE])
def test_late_issue_moves_its_requests_and_drops_none(asm, name, src):
    got, product = _lds_dma(_text(asm, name, src)), _lds_dma(_text(asm, "product", src))
    assert product > 0
    if src == "fa_fwd_pp.hip":
        assert got == product, (got, product)
    elif src in UNSTAGGERED:
        assert got == _lds_dma(_text(asm, "unstaggered", src)) and got < product, (got, _lds_dma(_text(asm, "unstaggered", src)), product)
    else:
        assert src == "fa_fwd_pp16.hip" and got >= product, (src, got, product)


@pytest.mark.parametrize("name,src", STAGE, ids=[f"{n}-{s[:-4]}" for n, s in STAGE])
def test_decode_variants_keep_the_launch_shape(asm, name, src):
    got, product = _resources(_text(asm, name, src)), _resources(_text(asm, "product", src))
    assert got.keys() == product.keys() and len(got) > 0
    changed = {k: (product[k], got[k]) for k in got if got[k] != product[k]}
    assert not changed, f"{name} / {src}: (scratch, LDS) product -> variant {changed}"
    assert all(s == 0 for s, _ in got.values())


def test_racy_form_moves_the_barrier_and_keeps_the_count(asm):
    """FA_KVC_STAGE_RACY puts the step's barrier in front of store_step: the same number of barriers as the slow-writer build (every wave still meets every barrier:
    nothing can hang), another text"""
    for src in fa_build.STAGE_SOURCES:
        racy, slow = _text(asm, "stage_racy_slow_writer", src), _text(asm, "stage_slow_writer", src)
        assert racy != slow and racy.count("s_barrier") == slow.count("s_barrier") == _text(asm, "product", src).count("s_barrier")
