"""GPU: flash_attn_merge_states / fa_run_merge_states against the fp64 merge of the same 16-bit inputs (tests/_merge_cases.py), and its exact relations.

Small on purpose: dense b 2, sq 3, h 5 (30 (row, head) pairs) and packed total 7 (35) - odd counts, so the last lane groups and the last wave are partial at
every d_v (8 / 16 / 32 / 64 lanes a pair) - every d_v, both dtypes, 2, 3 and 8 parts.  Every part lives in a larger buffer filled with NaN between rows, heads
and batch entries and past the last row, with strides of its own; one LSE of every call is the (batch, nheads, seqlen_q) view of a (1, nheads, batch * seqlen_q)
tensor.  The C-ABI runs write into guarded buffers that start as a pattern: nothing outside the extents may change."""
import math

import numpy as np
import pytest
import torch

import _merge_cases as M
import _util as U

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
LAYOUTS = {"dense": (2, 3, 5), "packed": (None, 7, 5)}          # (b, rows, h)
PARTS = (2, 3, 8)
NAN32 = float("nan")


def o_shape(layout, dv):
    b, rows, h = LAYOUTS[layout]
    return (rows, h, dv) if b is None else (b, rows, h, dv)


def l_shape(layout):
    b, rows, h = LAYOUTS[layout]
    return (h, rows) if b is None else (b, h, rows)


def make_parts(layout, dv, dtname, n, dev, seed, lse_lo=-30.0, lse_hi=30.0):
    """n parts in NaN-filled buffers, each with its own padding (= its own strides); lse gaps up to lse_hi - lse_lo; the last part's LSE in the
    (1, h, b * rows)-viewed form (dense) or transposed storage (packed)"""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    outs, lses = [], []
    b, rows, h = LAYOUTS[layout]
    for i in range(n):
        shape = o_shape(layout, dv)
        pad = tuple(2 * ((i + k) % 3) for k in range(len(shape) - 1)) + (16 + 8 * (i % 2),)
        _, view, _ = U.guarded(shape, DT[dtname], dev, pad)
        view.copy_(torch.randn(shape, generator=gen).to(dev))
        vals = (torch.rand(l_shape(layout), generator=gen) * (lse_hi - lse_lo) + lse_lo).to(dev)
        if i == n - 1 and b is not None:
            flat = torch.empty(1, h, b * rows, device=dev)
            l = flat.as_strided((b, h, rows), (rows, b * rows, 1))
        elif i == n - 1:
            l = torch.full((rows + 2, h + 1), NAN32, device=dev).t()[:h, 1:1 + rows]
        else:
            full = torch.full(tuple(s + 1 + (i + k) % 2 for k, s in enumerate(l_shape(layout))), NAN32, device=dev)
            l = full[tuple(slice(1, 1 + s) for s in l_shape(layout))]
        l.copy_(vals)
        assert tuple(view.shape) == shape and tuple(l.shape) == l_shape(layout)
        outs.append(view)
        lses.append(l)
    assert len({o.stride() for o in outs}) > 1 and len({l.stride() for l in lses}) > 1, "the parts must differ in their strides"
    return outs, lses


def run_capi(outs, lses):
    """the C ABI on guarded outputs that start as a pattern -> out, lse views (and asserts that nothing outside them changed)"""
    from flash_attn_turing import capi

    dev, dt = outs[0].device, outs[0].dtype
    obuf, out, osl = U.guarded(tuple(outs[0].shape), dt, dev, (2,) * (outs[0].dim() - 1) + (16,))
    lbuf = torch.full(tuple(s + 2 for s in lses[0].shape), -7.25, device=dev)
    lsl = tuple(slice(1, 1 + s) for s in lses[0].shape)
    lse = lbuf[lsl]
    o_before, l_before = obuf.clone(), lbuf.clone()
    capi.run_merge_states(capi.merge_params(outs, lses, out, lse, stream=torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    o_mask = torch.ones(obuf.shape, dtype=torch.bool, device=dev)
    o_mask[osl] = False
    l_mask = torch.ones(lbuf.shape, dtype=torch.bool, device=dev)
    l_mask[lsl] = False
    assert torch.equal(U.bits(obuf)[o_mask], U.bits(o_before)[o_mask]), "out: bytes outside the view changed"
    assert torch.equal(U.bits(lbuf)[l_mask], U.bits(l_before)[l_mask]), "lse: bytes outside the view changed"
    return out, lse


def run_both(outs, lses):
    """the Python function (new tensors) and the C ABI (guarded caller buffers) give the same bits -> out, lse"""
    from flash_attn_turing import flash_attn_merge_states

    out, lse = flash_attn_merge_states(outs, lses)
    out_c, lse_c = run_capi(outs, lses)
    assert out.is_contiguous() and lse.is_contiguous() and out.shape == outs[0].shape and lse.shape == lses[0].shape and lse.dtype == torch.float32
    assert torch.equal(U.bits(out), U.bits(out_c)) and torch.equal(U.bits(lse), U.bits(lse_c)), "Python function and C ABI differ"
    return out, lse


def to_rows(layout, o, l):
    """-> o (..rows.., h, d_v), lse (..rows.., h) float64 numpy in one row order for both"""
    o64 = o.double().cpu().numpy()
    l64 = l.double().cpu().numpy()
    return o64, (l64.T if LAYOUTS[layout][0] is None else np.transpose(l64, (0, 2, 1)))


def same_bits(a, b):
    return torch.equal(U.bits(a.contiguous()), U.bits(b.contiguous()))


@pytest.mark.parametrize("n", PARTS)
@pytest.mark.parametrize("dtname", ("fp16", "bf16"))
@pytest.mark.parametrize("dv", M.WIDTHS)
@pytest.mark.parametrize("layout", ("dense", "packed"))
def test_values_against_the_fp64_merge(gpu, layout, dv, dtname, n):
    """elementwise |out - ref| <= 2^-p |ref| + 2^-20 max_i |o_i| (+ 2^-25 for fp16 subnormals), |lse - ref| <= 2^-20 max(|ref|, 1); LSE gaps up to 60"""
    outs, lses = make_parts(layout, dv, dtname, n, gpu, 1000 * dv + 10 * n + (dtname == "bf16"))
    out, lse = run_both(outs, lses)
    po, pl = zip(*(to_rows(layout, o, l) for o, l in zip(outs, lses)))
    ref_o, ref_l = M.merge64(po, pl)
    got_o, got_l = to_rows(layout, out, lse)
    assert np.isfinite(got_o).all() and np.isfinite(got_l).all()
    gap = np.max(pl, axis=0) - np.min(pl, axis=0)
    assert gap.max() > (20 if n == 2 else 40), gap.max()
    err_o, err_l = np.abs(got_o - ref_o), np.abs(got_l - ref_l)
    bo, bl = M.out_bound(ref_o, po, dtname), M.lse_bound(ref_l)
    print(f"merge {layout} d_v {dv} {dtname} n {n}: worst out err / bound {float((err_o / bo).max()):.3f}, lse err / bound {float((err_l / bl).max()):.3f}, max gap {gap.max():.1f}")
    assert (err_o <= bo).all(), (float((err_o / bo).max()), np.unravel_index((err_o / bo).argmax(), err_o.shape))
    assert (err_l <= bl).all(), float((err_l / bl).max())


@pytest.mark.parametrize("dtname", ("fp16", "bf16"))
@pytest.mark.parametrize("dv", M.WIDTHS)
def test_a_part_among_empty_parts_comes_back_bit_for_bit(gpu, dv, dtname):
    """both empty forms - lse = -inf (its o rows hold NaN: never read into a result) and the library's dead row (lse = +-0, o = +-0) - in every argument
    position, 2, 3 and 8 parts, dense and packed; all parts empty is out = 0, lse = 0"""
    for layout in LAYOUTS:
        for n in PARTS:
            outs, lses = make_parts(layout, dv, dtname, n, gpu, 77 + n)
            live_o, live_l = outs[0].clone(), lses[0].clone()
            for form in ("ninf", "dead", "mixed"):
                for pos in range(n):
                    for i in range(n):
                        if i == pos:
                            outs[i].copy_(live_o); lses[i].copy_(live_l)
                        elif form == "ninf" or (form == "mixed" and i % 2):
                            outs[i].fill_(float("nan")); lses[i].fill_(float("-inf"))
                        else:
                            outs[i].zero_(); lses[i].zero_()
                            outs[i][..., 1::2] = -0.0                                     # +-0 alike
                            lses[i][..., ::2] = -0.0
                    out, lse = run_both(outs, lses)
                    assert same_bits(out, live_o) and same_bits(lse, live_l), (layout, n, form, pos)
            for i in range(n):
                if i % 2:
                    outs[i].fill_(float("nan")); lses[i].fill_(float("-inf"))
                else:
                    outs[i].zero_(); lses[i].zero_()
            out, lse = run_both(outs, lses)
            assert (U.bits(out) == 0).all().item() and (U.bits(lse) == 0).all().item(), (layout, n, "all parts empty must be out = +0, lse = +0")
            # a merged dead row feeds another merge as an empty part
            outs[0].copy_(live_o); lses[0].copy_(live_l)
            out2, lse2 = run_both([outs[0], out] + list(outs[2:]), [lses[0], lse] + list(lses[2:]))
            assert same_bits(out2, live_o) and same_bits(lse2, live_l), (layout, n, "merge of a merge")


@pytest.mark.parametrize("dtname", ("fp16", "bf16"))
@pytest.mark.parametrize("dv", M.WIDTHS)
def test_two_copies_of_one_part(gpu, dv, dtname):
    """weights 1 and 1: out is the part's bits ((o + o) / 2 is exact), lse is lse + log 2 within the LSE rule"""
    for layout in LAYOUTS:
        outs, lses = make_parts(layout, dv, dtname, 2, gpu, 5)
        outs[1].copy_(outs[0]); lses[1].copy_(lses[0])
        out, lse = run_both(outs, lses)
        assert same_bits(out, outs[0]), layout
        ref = lses[0].double().cpu().numpy() + math.log(2.0)
        assert (np.abs(lse.double().cpu().numpy() - ref) <= M.lse_bound(ref)).all(), layout


@pytest.mark.parametrize("dtname", ("fp16", "bf16"))
@pytest.mark.parametrize("dv", M.WIDTHS)
def test_a_nan_stays_in_its_row_and_head(gpu, dv, dtname):
    """a NaN lse_i, or one NaN element in a non-empty part's row, makes that (row, head) NaN - every element of out, and lse - and leaves the bits of every
    other (row, head) as they were; a NaN in an EMPTY part's row changes nothing"""
    for layout in LAYOUTS:
        b, rows, h = LAYOUTS[layout]
        for n in PARTS:
            outs, lses = make_parts(layout, dv, dtname, n, gpu, 31 * n)
            base_o, base_l = run_both(outs, lses)
            hit = (rows - 1, h - 2) if b is None else (1, rows - 1, h - 2)            # (.., row, head): in the last, partial wave
            l_hit = (h - 2, rows - 1) if b is None else (1, h - 2, rows - 1)
            for part in sorted({0, n - 1}):
                for what in ("lse", "o", "o_empty"):
                    o_keep, l_keep = outs[part].clone(), lses[part].clone()
                    if what == "lse":
                        lses[part][l_hit] = float("nan")
                    else:
                        outs[part][hit + (dv - 3,)] = float("nan")
                        if what == "o_empty":
                            lses[part][l_hit] = float("-inf")
                    out, lse = run_both(outs, lses)
                    if what == "o_empty":
                        outs[part].copy_(o_keep)                                        # the same call without the NaN: the part is empty there either way
                        ref_o, ref_l = run_both(outs, lses)
                        assert same_bits(out, ref_o) and same_bits(lse, ref_l), (layout, n, part, what)
                    else:
                        assert torch.isnan(out[hit]).all().item() and torch.isnan(lse[l_hit]).item(), (layout, n, part, what)
                        keep_o = torch.ones(out.shape[:-1], dtype=torch.bool, device=gpu)
                        keep_o[hit] = False
                        keep_l = torch.ones(lse.shape, dtype=torch.bool, device=gpu)
                        keep_l[l_hit] = False
                        assert torch.equal(U.bits(out)[keep_o], U.bits(base_o)[keep_o]) and torch.equal(U.bits(lse)[keep_l], U.bits(base_l)[keep_l]), (layout, n, part, what)
                    outs[part].copy_(o_keep); lses[part].copy_(l_keep)


def test_large_call_and_graph_replay(gpu):
    """more than one workgroup per d_v and a row index past one block (b 3, sq 171, h 5 = 2565 pairs), captured and replayed with new contents: the call
    allocates its outputs but synchronises nothing"""
    from flash_attn_turing import flash_attn_merge_states

    gen = torch.Generator(device="cpu").manual_seed(9)
    outs = [torch.randn(3, 171, 5, 128, generator=gen).to(gpu, torch.bfloat16) for _ in range(3)]
    lses = [(torch.rand(3, 5, 171, generator=gen) * 20 - 10).to(gpu) for _ in range(3)]
    eager = flash_attn_merge_states(outs, lses)
    ref_o, ref_l = M.merge64([o.double().cpu().numpy() for o in outs], [l.double().cpu().numpy().transpose(0, 2, 1) for l in lses])
    assert (np.abs(eager[0].double().cpu().numpy() - ref_o) <= M.out_bound(ref_o, [o.double().cpu().numpy() for o in outs], "bf16")).all()
    assert (np.abs(eager[1].double().cpu().numpy().transpose(0, 2, 1) - ref_l) <= M.lse_bound(ref_l)).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        flash_attn_merge_states(outs, lses)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = flash_attn_merge_states(outs, lses)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(got[0], eager[0]) and same_bits(got[1], eager[1])
    outs[1].copy_(torch.randn(3, 171, 5, 128, generator=gen).to(gpu, torch.bfloat16))
    lses[2].add_(3.0)
    graph.replay()
    torch.cuda.synchronize()
    again = flash_attn_merge_states(outs, lses)
    assert same_bits(got[0], again[0]) and same_bits(got[1], again[1]) and not same_bits(got[0], eager[0])
