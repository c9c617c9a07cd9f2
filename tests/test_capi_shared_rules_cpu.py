"""The argument rules that several entry points of the C ABI share (fa_capi.hip states each once): every entry point that has a rule refuses the same mistake
with the same code and the same words.  The words are those the library has always used; where the entry points differ on purpose (the default a scale of 0
stands for, the wording of a missing header, the code of a non-zero reserved_ field, an empty workspace) the difference is spelled out here.
No GPU: every call is refused, or returns for an empty batch, before anything is launched."""
import ctypes

import pytest

from flash_attn_turing import capi

PAGE = 64


def _aligned():
    """a fake device address, 16-byte aligned (never dereferenced by the host checks)"""
    _aligned.next += 1 << 20
    return _aligned.next


_aligned.next = 0x7F0000000000


def _kvcache():
    p = capi.KvcacheParams()
    p.seqlen_q, p.seqlen_cache, p.h, p.h_k, p.d = 1, 4 * PAGE, 8, 2, 128
    return p


def _mla():
    p = capi.MlaParamsV2()
    p.seqlen_q, p.seqlen_cache, p.h, p.d_qk, p.d_v = 1, 4 * PAGE, 16, 576, 512
    return p


def _sparse():
    p = capi.MlaSparseParamsV2()
    p.seqlen_q, p.seqlen_cache, p.h, p.d_qk, p.d_v, p.topk = 1, 4 * PAGE, 16, 576, 512, 64
    return p


def _indexer():
    p = capi.MlaIndexerParams()
    p.seqlen_q, p.seqlen_cache, p.h, p.d = 1, 4 * PAGE, 32, 128
    return p


def _topk():
    p = capi.MlaTopkParams()
    p.seqlen_q, p.seqlen_cache, p.topk = 1, 4 * PAGE, 64
    return p


def _dense(cls, **kw):
    p = cls()
    p.seqlen_q, p.seqlen_k, p.h, p.h_k = 8, 8, 4, 2
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _merge():
    p = capi.MergeParams()
    p.n_parts, p.d_v = 2, 128
    return p


def _call(name, *extra):
    def call(p, options=None):
        args = (ctypes.byref(p) if p is not None else None,) + ((ctypes.byref(options) if options is not None else None,) if "_ex" in name else ()) + extra
        return getattr(capi.lib(), name)(*args)
    return call


# entry point -> (a valid struct of an empty batch, the call that validates it with the workspace fields looked at, the struct's name in messages)
ENTRY = {
    "fwd": (lambda: _dense(capi.FwdParams, d=64), _call("fa_run_mha_fwd", None), "fa_fwd_params"),
    "bwd": (lambda: _dense(capi.BwdParams, d=64), _call("fa_bwd_dkdv", None), "fa_bwd_params"),
    "kvcache": (_kvcache, _call("fa_kvcache_num_splits_ex"), "fa_kvcache_params"),
    "mla": (_mla, _call("fa_mla_num_splits"), "fa_mla_params"),
    "mla_sparse": (_sparse, _call("fa_mla_sparse_num_splits"), "fa_mla_sparse_params"),
    "indexer": (_indexer, _call("fa_run_mla_indexer_logits", None), "fa_mla_indexer_params"),
    "topk": (_topk, _call("fa_run_mla_indexer_topk", None), "fa_mla_topk_params"),
    "prefill": (lambda: _dense(capi.MlaPrefillParams, d_qk=192, d_v=128), _call("fa_run_mla_prefill_fwd", None), "fa_mla_prefill_params"),
    "prefill_bwd": (lambda: _dense(capi.MlaPrefillBwdParams, d_qk=192, d_v=128), _call("fa_run_mla_prefill_bwd", None), "fa_mla_prefill_bwd_params"),
    "merge": (_merge, _call("fa_run_merge_states"), "fa_merge_params"),
}


def _refused(entry, code, words, options=None, **fields):
    make, call, _ = ENTRY[entry]
    p = make()
    for k, v in fields.items():
        setattr(p, k, v)
    rc = call(p, options) if options is not None else call(p)
    assert (rc, capi.last_error()) == (code, words), (entry, fields)


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_every_struct_is_valid_before_it_is_broken(entry):
    make, call, _ = ENTRY[entry]
    assert call(make()) >= 0, capi.last_error()


PAGED_MISTAKES = [      # (fields on top of a valid paged struct, code, words) - the list of test_kvcache_paged_cpu.py::test_paged_validation_codes, in full words
    (dict(page_block_size=0), capi.FA_ERR_BAD_SHAPE, "block_table given without page_block_size"),
    (dict(page_block_size=8, seqlen_cache=64), capi.FA_ERR_BAD_SHAPE, "page_block_size 8 must be a positive multiple of 16"),
    (dict(page_block_size=40, seqlen_cache=80), capi.FA_ERR_BAD_SHAPE, "page_block_size 40 must be a positive multiple of 16"),
    (dict(page_block_size=-16, seqlen_cache=64), capi.FA_ERR_BAD_SHAPE, "page_block_size -16 must be a positive multiple of 16"),
    (dict(num_blocks=0), capi.FA_ERR_BAD_SHAPE, "num_blocks 0: a paged cache needs at least one page"),
    (dict(num_blocks=-3), capi.FA_ERR_BAD_SHAPE, "num_blocks -3: a paged cache needs at least one page"),
    (dict(seqlen_cache=1000), capi.FA_ERR_BAD_SHAPE, "seqlen_cache (1000) must be a positive multiple of page_block_size (64) with block_table"),
    (dict(seqlen_cache=0), capi.FA_ERR_BAD_SHAPE, "seqlen_cache (0) must be a positive multiple of page_block_size (64) with block_table"),
    (dict(seqlen_cache=4096, block_table_stride=63), capi.FA_ERR_BAD_STRIDE, "block_table_stride 63 is below the table's 64 columns (seqlen_cache / page_block_size)"),
    (dict(block_table=0x7F0000000002), capi.FA_ERR_BAD_STRIDE, "block_table must be 4-byte aligned"),
    (dict(block_table=None, page_block_size=16), capi.FA_ERR_NULL_POINTER, "page_block_size = 16 given without block_table"),
]


@pytest.mark.parametrize("entry", ["kvcache", "mla", "mla_sparse", "indexer"])
def test_paged_block(entry):
    paged = dict(block_table=_aligned(), block_table_stride=4, page_block_size=PAGE, num_blocks=9)
    make, call, _ = ENTRY[entry]
    p = make()
    for k, v in paged.items():
        setattr(p, k, v)
    assert call(p) >= 0, capi.last_error()
    for fields, code, words in PAGED_MISTAKES:
        _refused(entry, code, words, **dict(paged, **fields))


@pytest.mark.parametrize("entry", ["kvcache", "mla", "mla_sparse", "bwd"])
def test_workspace_pair(entry):
    _refused(entry, capi.FA_ERR_BAD_SHAPE, "workspace_bytes must be >= 0", workspace=_aligned(), workspace_bytes=-1)
    _refused(entry, capi.FA_ERR_BAD_SHAPE, "workspace_bytes must be >= 0", workspace=None, workspace_bytes=-1)
    _refused(entry, capi.FA_ERR_BAD_STRIDE, "workspace must be 16-byte aligned", workspace=_aligned() + 8, workspace_bytes=4096)
    # kept on purpose: fa_bwd_params does not look at the pointer of an empty workspace, the decode structs refuse a misaligned one of any size
    make, call, _ = ENTRY[entry]
    p = make()
    p.workspace, p.workspace_bytes = _aligned() + 8, 0
    if entry == "bwd":
        assert call(p) == capi.FA_OK
    else:
        assert (call(p), capi.last_error()) == (capi.FA_ERR_BAD_STRIDE, "workspace must be 16-byte aligned")


def test_workspace_pair_is_not_looked_at_by_the_workspace_queries():
    L = capi.lib()
    for make, fn in ((_kvcache, L.fa_kvcache_workspace_bytes), (_mla, L.fa_mla_workspace_bytes), (_sparse, L.fa_mla_sparse_workspace_bytes),
                     (lambda: _dense(capi.BwdParams, d=64), L.fa_bwd_workspace_bytes)):
        p = make()
        p.workspace, p.workspace_bytes = _aligned() + 8, -1
        assert fn(ctypes.byref(p)) == 0, capi.last_error()


@pytest.mark.parametrize("entry", ["kvcache", "mla", "mla_sparse"])
def test_num_splits(entry):
    for n in (-1, -2**31):
        _refused(entry, capi.FA_ERR_BAD_SHAPE, f"num_splits must be >= 0 (0 = the library's choice), got {n}", num_splits=n)


@pytest.mark.parametrize("entry", ["fwd", "bwd", "kvcache", "mla", "mla_sparse", "indexer", "prefill", "prefill_bwd", "merge"])
def test_dtype(entry):
    for dtype in (2, 7, -1):
        _refused(entry, capi.FA_ERR_BAD_DTYPE, f"dtype {dtype} unsupported (0=fp16, 1=bf16)", dtype=dtype)


SCALE_DEFAULT = {"kvcache": "1 / sqrt(head_dim)", "mla": "576 ** -0.5", "mla_sparse": "576 ** -0.5", "prefill": "192 ** -0.5", "prefill_bwd": "192 ** -0.5"}


@pytest.mark.parametrize("entry", sorted(SCALE_DEFAULT))
def test_softmax_scale(entry):
    for scale, shown in ((-1.0, "-1"), (float("inf"), "inf"), (float("-inf"), "-inf"), (float("nan"), None)):
        words = f"softmax_scale {shown} must be finite and > 0 (0 = the default {SCALE_DEFAULT[entry]})"
        make, call, _ = ENTRY[entry]
        p = make()
        if entry == "kvcache":          # the scale of the decode call is a field of its options
            o = capi.KvcacheOptionsV5()
            o.softmax_scale = scale
            rc = call(p, o)
        else:
            p.softmax_scale = scale
            rc = call(p)
        assert rc == capi.FA_ERR_BAD_SHAPE, (entry, scale)
        if shown is None:               # (the sign printf gives a NaN is the C library's)
            assert capi.last_error().replace("-nan", "nan") == words.replace("None", "nan")
        else:
            assert capi.last_error() == words


@pytest.mark.parametrize("entry", sorted(ENTRY))
def test_header(entry):
    make, call, what = ENTRY[entry]
    assert (call(None), capi.last_error()) == (capi.FA_ERR_NULL_POINTER, "params is NULL")
    # the structs that are older than FA_PARAMS_INIT, or grew, word a wrong magic as an old caller's; the one-size structs as a missing initialisation: both stay
    if entry in ("fwd", "bwd", "kvcache", "mla", "mla_sparse"):
        words = f"{what}: no {{struct_size, magic}} header - caller was compiled against an ABI < 4 header; recompile against include/flash_attn_gfx950.h (ABI 4)"
    else:
        words = f"{what}: magic is not FA_PARAMS_MAGIC - no {{struct_size, magic}} header; initialise the struct with FA_PARAMS_INIT (ABI 4)"
    for magic in (0, capi.FA_PARAMS_MAGIC ^ 1):
        _refused(entry, capi.FA_ERR_BAD_ABI, words, magic=magic)
    p = make()
    p.struct_size = ctypes.sizeof(p) + 8
    assert call(p) == capi.FA_ERR_BAD_ABI and capi.last_error().startswith(f"{what}: struct_size {ctypes.sizeof(p) + 8} ")


RESERVED_CODE = {"mla": capi.FA_ERR_BAD_ABI, "mla_sparse": capi.FA_ERR_BAD_ABI, "indexer": capi.FA_ERR_BAD_SHAPE, "topk": capi.FA_ERR_BAD_SHAPE,
                 "prefill_bwd": capi.FA_ERR_BAD_SHAPE}


@pytest.mark.parametrize("entry", sorted(RESERVED_CODE))
def test_reserved_field(entry):
    """one rule, one wording; the code is the one each struct shipped with (FA_ERR_BAD_ABI in the two MLA decode structs, FA_ERR_BAD_SHAPE in those after them)"""
    _refused(entry, RESERVED_CODE[entry], f"{ENTRY[entry][2]}: reserved_ is not zero (a field of a newer header that this library does not know)", reserved_=1)
