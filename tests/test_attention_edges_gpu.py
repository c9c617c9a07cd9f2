"""GPU: dense and packed attention (fwd / bwd / varlen_fwd / varlen_bwd) at its edges, under both kernel sets.

Every test runs twice, with the 16x16x32 and the 32x32x16 kernel set pinned (fixture `pinned_set`), and compares launches of the same shape
only: the default policy picks kernels by shape and CU count, so a smaller launch is a different kernel.
  A. late softmax spikes in the tiles the fp16 16x16x32 forward sums through the matrix pipe (fa_fwd_pp16.hip: FA_PP16_MFMA_ROWSUM), where
     the optimistic pass is guarded by the largest packed P of each lane; one spike per wave and tile, because the refresh decision is a
     wave-wide ballot: a second spike in the same wave and tile would fire the refresh for a word the guard missed;
  B. NaN and +-inf in Q and K against fp64 math on the same bits (U.fp64_math): NaN pattern, untouched rows bit for bit, dead rows;
  C. memory outside the problem (gaps between rows, heads and batch entries, rows past each entry or past cu_seqlens[-1], padded LSE and
     dsoftmax_sum entries, the dK/dV workspace) holds NaN, +-inf and 65504 and is never read into a result;
  D. one item (batch entry, packed sequence, KV head with its query heads, one query head) filled with NaN leaves every other item's bits;
  E. outputs are views into sentinel-filled buffers: nothing outside them is written, everything inside is.
Non-finite V and a non-finite backward have no exact contract (within a key tile a masked P = 0 still multiplies V, and 0 x NaN is NaN;
include/flash_attn_gfx950.h) and are not tested here."""

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
SENT32 = 0x7FA5A5A5      # an fp32 NaN payload nobody computes
BLOCK_M = 256            # query rows per workgroup of the 16x16x32 forward (fwd_pp16_block_m, both head dims)
NAN_BITS = {"fp16": (0x7E00, 0xFE00), "bf16": (0x7FC0, 0xFFC0)}      # quiet NaN with the sign bit clear / set
INF_BITS = {"fp16": 0x7C00, "bf16": 0x7F80}


@pytest.fixture(autouse=True, params=["mfma16", "mfma32"])
def pinned_set(gpu, request):
    prev = capi.set_kernel_policy(capi.POLICY_MFMA16 if request.param == "mfma16" else capi.POLICY_MFMA32)
    yield request.param
    capi.set_kernel_policy(prev)


def _rand(shape, dt, gen, dev, scale=1.0):
    return (torch.randn(*shape, device=dev, dtype=torch.float32, generator=gen) * scale).to(dt)


def _same(a, b):
    return torch.equal(U.bits(a), U.bits(b))


def _s32(n, dev):
    """n fp32 sentinel values"""
    return torch.full((n,), SENT32, dtype=torch.int32, device=dev).view(torch.float32)


def _set_bits(t, idx, pattern):
    """write a 16-bit pattern into one element of a 16-bit tensor"""
    t.view(torch.int16)[idx] = pattern - 0x10000 if pattern >= 0x8000 else pattern


# ---- geometry of the 16x16x32 forward (fa_fwd_pp16.hip) ------------------------------------------------------------------------------

def _pp16_tiles(d):
    """(keys per tile, first matrix-summed tile): FA_PP16_EXACT_TILES = 16 tiles of 64 keys, counted in tiles of the instance, rounded up
    to the start of a three-tile trip (kExact)"""
    bn = 64 if d == 128 else 128
    exact_tiles = 16 * 64 // bn
    return bn, 1 + 3 * ((exact_tiles + 1) // 3)


def _ml_tiles(d, sq, sk, causal, m0):
    """key tiles the fp16 16x16x32 forward sums through the matrix pipe for the workgroup whose first query row is m0 (fa_fwd_pp16.hip,
    set_current and the steady loop): whole three-tile trips from kExact on, inside the n_main tiles that every row of the workgroup sees
    whole; the last one or two steady tiles, and the masked / ragged ones after them, are summed exactly"""
    bn, k_exact = _pp16_tiles(d)
    n_tiles = -(-sk // bn)
    if causal:
        max_key = min(m0 + BLOCK_M, sq) - 1 + sk - sq
        n_tiles = 0 if max_key < 0 else min(n_tiles, max_key // bn + 1)
    n_main = min(n_tiles, sk // bn)
    if causal:
        n_main = min(n_main, max(0, (m0 + sk - sq + 1) // bn))
    if n_main < k_exact + 3:
        return range(0)
    return range(k_exact, k_exact + 3 * ((n_main - k_exact) // 3))


# ---- A. late softmax spikes ----------------------------------------------------------------------------------------------------------

_ORACLE = {}


def _close(x, ref, dtype, name, sk, oracle_of, scale=1.0):
    """U.assert_close against fp32 math; the plain mean_rel bound first, and only where the kernel misses it the C oracle's bound
    (U.check_mean_rel: max(1e-2, 2 x the reference algorithm's own error)), whose result is computed once per problem"""
    try:
        U.assert_close(x, ref, dtype, name, scale=scale, sk=sk)
    except AssertionError as e:
        if "mean_rel" not in str(e) or "max_abs" in str(e) or "mean_abs" in str(e):
            raise
        U.assert_close(x, ref, dtype, name, scale=scale, sk=sk, oracle=oracle_of())


def _spike_problem(dtype, d, causal, height, gpu):
    """b x h slots of one 256-row workgroup; slot s hosts the tests T = 16 s .. 16 s + 15: test T puts one key at tile kExact + T % 16,
    key position T % BN, for the row of wave T % 8 at query column T // BN (rows n and n + 16 of a lane), column position varying.  Each
    wave gets one spike per tile and each row at most one, and the tests cover every (query column, key position) pair: every packed
    word of every lane's guard chain.  The 32 rows of a wave are orthogonal (q = sqrt(d) x orthonormal rows), so a spike key scores
    only its own row above the rest of its wave."""
    dt = DT[dtype]
    bn, k_exact = _pp16_tiles(d)
    n_ml, sq, h = 16, BLOCK_M, 8
    b = 2 * bn // (h * n_ml)
    need_main = k_exact + 3 * (-(-n_ml // 3))
    sk = need_main * bn + 37 + (sq - 1 if causal else 0)            # + a ragged tile; causal: the first row still sees need_main tiles
    ml = _ml_tiles(d, sq, sk, causal, 0)
    gen = torch.Generator(device="cpu").manual_seed(1000 + d + 7 * int(causal) + int(height))
    basis = torch.linalg.qr(torch.randn(b * h * (sq // 32), d, 32, generator=gen))[0]           # (waves, d, 32) orthonormal columns
    q = (basis.transpose(1, 2).reshape(b, h, sq, d).permute(0, 2, 1, 3) * d ** 0.5).to(dt).float()
    k = torch.randn(b, sk, h, d, generator=gen).to(dt).float()
    v = torch.randn(b, sk, h, d, generator=gen)
    do = torch.randn(b, sq, h, d, generator=gen)
    spikes = []
    for s in range(b * h):
        bi, hh = divmod(s, h)
        for i in range(n_ml):
            t = s * n_ml + i
            kp, col, wave = t % bn, t // bn, t % 8
            n = (5 * i + 3 * s) % 16
            row = 32 * wave + 16 * col + n
            tile = k_exact + i
            key = tile * bn + kp
            assert tile in ml, (tile, ml)                       # the spike lies in a matrix-summed tile of this workgroup
            assert key <= row + sk - sq                          # ... and the row sees it
            spikes.append((bi, hh, row, key))
    assert len(spikes) == 2 * bn and len({(x[0], x[1], x[2]) for x in spikes}) == len(spikes)
    for bi, hh, row, key in spikes:
        qr = q[bi, row, hh]
        level = (k[bi, :row + sk - sq + 1 if causal else sk, hh] @ qr).max() / d ** 0.5
        u = qr / qr.norm()
        kj = k[bi, key, hh]
        k[bi, key, hh] = kj - (kj @ u) * u + (level + height) * d ** 0.5 / qr.norm() * u
    q, k, v, do = (x.to(gpu, dt) for x in (q, k, v, do))
    return q, k, v, do, sk, spikes


@pytest.mark.parametrize("height", [8.0, 30.0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_late_spikes_in_matrix_summed_tiles(gpu, dtype, d, causal, height, pinned_set):
    """One key per tested row scores `height` nats above the rest of its row, in a tile past the exactly summed prefix: 8 nats (P still
    fits fp16, the guard must fire the refresh) and 30 (P overflows fp16 if it does not).  O within the suite's tolerance of fp32 math,
    LSE within U.LSE_TOL, everything finite; the backward on the same inputs likewise (dQ: see below)."""
    q, k, v, do, sk, spikes = _spike_problem(dtype, d, causal, height, gpu)
    b, sq, h, _ = q.shape
    if pinned_set == "mfma16":
        assert capi.kernel_name("fwd", b, sq, sk, h, d, causal, dtype) == "fa_fwd_pp16_kernel"
    o, lse = F.fwd(q, k, v, causal)
    dq, dk, dv = F.bwd(q, k, v, o, lse, do, causal)
    o_r, lse_r, dq_r, dk_r, dv_r = U.torch_attention_ref(q, k, v, do, causal)
    for name, x in (("O", o), ("LSE", lse), ("dQ", dq), ("dK", dk), ("dV", dv)):
        assert torch.isfinite(x).all().item(), f"{name}: non-finite values"
    lse_s = torch.tensor([lse_r[bi, hh, row].item() - (q[bi, row, hh].float() @ k[bi, key, hh].float()).item() / d ** 0.5
                          for bi, hh, row, key in spikes])
    assert (lse_s.abs() < 1.0).all(), "each tested row's LSE must be its spike's score: the spike dominates the row"
    assert (lse - lse_r).abs().max().item() <= U.LSE_TOL

    key = (dtype, d, causal, height)

    def oracle(i):
        def get():
            if key not in _ORACLE:
                from oracle import attn_oracle as A

                mode = A.ROUND_FP16 if dtype == "fp16" else A.ROUND_BF16
                n = lambda t: t.float().cpu().numpy()
                oo, ol = A.attn_fwd(n(q), n(k), n(v), causal=causal, round_mode=mode)
                _ORACLE[key] = (oo,) + tuple(A.attn_bwd(n(q), n(k), n(v), oo, ol, n(do), causal=causal, round_mode=mode))
            return _ORACLE[key][i]
        return get

    tag = f"spikes {height} {dtype} d{d} causal={causal} {pinned_set}"
    for i, (name, x, r) in zip((0, 2, 3), (("O", o, o_r), ("dK", dk, dk_r), ("dV", dv, dv_r))):
        _close(x.float().cpu().numpy(), r.cpu().numpy(), dtype, f"{name} {tag}", sk, oracle(i))
    # dQ.  A row whose spike carries all but e^-30 of its weight has dQ = sum_j P_j (dP_j - D) K_j ~ 0 (|dQ| < 1e-6 in fp64): there ANY
    # fp32 implementation leaves the noise of dP_s - D (the suite's "zero" rule, U.ZERO_ABS_TOL).  Elsewhere the big spike keys meet rows
    # of other waves at moderate weight, |dQ| reaches ~17, and the reference algorithm itself (C oracle: dS rounded to 16 bits before
    # dQ = dS K) is 8.2e-3 off fp32 math in max_abs at head_dim 64: those rows get twice the plain bounds, and the oracle's mean_rel rule.
    spiked = torch.zeros(b, sq, h, dtype=torch.bool)
    for bi, hh, row, _ in spikes:
        spiked[bi, row, hh] = True
    xq, rq = dq.float().cpu(), dq_r.cpu()
    rest = torch.ones_like(spiked)
    if height >= 30.0:
        # (a few rows meet other waves' spike keys before their own at head_dim 64, which leaves their spike ~11 nats clear: not vanishing)
        vanish = spiked & (rq.abs().amax(-1) < 1e-6)
        assert vanish.sum().item() >= len(spikes) // 2, "most 30-nat rows' dQ must vanish"
        zmax = xq[vanish].abs().max().item()
        assert zmax <= U.ZERO_ABS_TOL, f"dQ {tag}: rows whose dQ vanishes, kernel max |x| = {zmax:.3e} > {U.ZERO_ABS_TOL:.1e}"
        rest = ~vanish
    _close(xq[rest].numpy(), rq[rest].numpy(), dtype, f"dQ {tag}", sk, lambda: oracle(1)()[rest.numpy()], scale=2.0)


# ---- B. non-finite Q and K -----------------------------------------------------------------------------------------------------------

def _nonfinite_layout(layout, d, dt, gen, gpu):
    """q, k, v, cu_q, cu_k (None: dense) and the places of the bad K element: (entry, key, kv head), one per (entry, kv head) pair.
    The long entries have 300 queries over 2000 keys: the exact prefix, a matrix-summed tile, the causal diagonal (key delta + 100:
    query rows below 100 cannot see it) and the ragged last tile.  Packed: a short neighbour with more queries than keys (causal: its
    first 30 rows see no key)."""
    bn, k_exact = _pp16_tiles(d)
    h, hk = 4, 2
    lq, lk = ([300, 300], [2000, 2000]) if layout == "dense" else ([300, 70, 300], [2000, 40, 2000])
    ml_key = (k_exact + 1) * bn + 5
    long_ = [i for i, L in enumerate(lk) if L == 2000]
    places = [(long_[0], 70, 0), (long_[0], ml_key, 1), (long_[1], 2000 - 300 + 100, 0), (long_[1], 1999, 1)]
    for causal in (False, True):
        assert (k_exact + 1) in _ml_tiles(d, 300, 2000, causal, 0), "the matrix-summed placement must reach such a tile"
    if layout == "dense":
        q, k, v = _rand((2, 300, h, d), dt, gen, gpu), _rand((2, 2000, hk, d), dt, gen, gpu), _rand((2, 2000, hk, d), dt, gen, gpu)
        return q, k, v, None, None, lq, lk, places
    cu_q = torch.tensor(np.concatenate([[0], np.cumsum(lq)]).astype(np.int32), device=gpu)
    cu_k = torch.tensor(np.concatenate([[0], np.cumsum(lk)]).astype(np.int32), device=gpu)
    q, k, v = _rand((sum(lq), h, d), dt, gen, gpu), _rand((sum(lk), hk, d), dt, gen, gpu), _rand((sum(lk), hk, d), dt, gen, gpu)
    return q, k, v, cu_q, cu_k, lq, lk, places


def _entry(t, cu, i):
    return t[i] if cu is None else t[int(cu[i]):int(cu[i + 1])]


def _fwd(q, k, v, cu_q, cu_k, lq, lk, causal):
    if cu_q is None:
        return F.fwd(q, k, v, causal)
    return F.varlen_fwd(q, k, v, cu_q, cu_k, max(lq), max(lk), causal)


@pytest.mark.parametrize("case", ["q_nan", "k_nan", "k_nan_signed", "k_inf"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("layout", ["dense", "packed"])
@pytest.mark.parametrize("dtype,d", [("fp16", 128), ("bf16", 128), ("fp16", 64), ("bf16", 64)])
def test_nonfinite_q_and_k_follow_fp64_math(gpu, dtype, d, layout, causal, case, pinned_set):
    """A NaN in one Q element, a NaN in one K element (sign bit clear / set) or a +inf in one K element (score +inf - a NaN row - where
    the query component is positive, -inf - the key drops out - where it is negative), in the exact prefix, in a matrix-summed tile, in
    the causal diagonal tile just past some rows' last key, and in the ragged last tile: the NaN pattern of O and LSE is that of fp64 math
    on the same bits, never +-inf; rows that cannot see the bad value keep the clean run's bits, except the other rows of a 32-row wave
    with a +inf score (the forward refreshes its running max per wave: they round P differently); those and the rows that lost a key
    match fp64 math; rows that see no key stay O = 0, LSE = 0 (a NaN query included); a rerun gives the same bits."""
    dt = DT[dtype]
    gen = torch.Generator(device=gpu).manual_seed(3000 + d + 11 * int(causal) + 5 * len(case))
    q, k, v, cu_q, cu_k, lq, lk, places = _nonfinite_layout(layout, d, dt, gen, gpu)
    qb, kb = q.clone(), k.clone()
    if case == "q_nan":
        for i, t, hq, c in ((0, 5, 0, 3), (len(lq) - 1, 299, 3, 40), (len(lq) - 1, 170, 1, 0)) + (((1, 3, 2, 9),) if layout == "packed" else ()):
            idx = (i, t, hq, c) if cu_q is None else (int(cu_q[i]) + t, hq, c)
            _set_bits(qb, idx, NAN_BITS[dtype][0])
    else:
        pattern = {"k_nan": NAN_BITS[dtype][0], "k_nan_signed": NAN_BITS[dtype][1], "k_inf": INF_BITS[dtype]}[case]
        for i, j, g in places:
            idx = (i, j, g, 7 + j % 50) if cu_k is None else (int(cu_k[i]) + j, g, 7 + j % 50)
            _set_bits(kb, idx, pattern)
    o_c, l_c = _fwd(q, k, v, cu_q, cu_k, lq, lk, causal)
    o_b, l_b = _fwd(qb, kb, v, cu_q, cu_k, lq, lk, causal)
    o_b2, l_b2 = _fwd(qb, kb, v, cu_q, cu_k, lq, lk, causal)
    assert _same(o_b, o_b2) and _same(l_b, l_b2), "not deterministic"
    tag = f"{case} {layout} {dtype} d{d} causal={causal} {pinned_set}"
    n_nan, n_lost = 0, 0
    for i in range(len(lq)):
        xo, xl, co, cl = _entry(o_b, cu_q, i), l_b[i, :, :lq[i]], _entry(o_c, cu_q, i), l_c[i, :, :lq[i]]
        ro, rl = U.fp64_math(_entry(qb, cu_q, i), _entry(kb, cu_k, i), _entry(v, cu_k, i), causal, device=gpu)
        ro_c, rl_c = U.fp64_math(_entry(q, cu_q, i), _entry(k, cu_k, i), _entry(v, cu_k, i), causal, device=gpu)
        assert not torch.isinf(xo).any().item() and not torch.isinf(xl).any().item(), f"{tag}: +-inf in entry {i}"
        assert torch.equal(torch.isnan(xl), torch.isnan(rl)), f"{tag}: entry {i} LSE NaN pattern {torch.isnan(xl).nonzero().tolist()[:8]} != fp64 {torch.isnan(rl).nonzero().tolist()[:8]}"
        assert torch.equal(torch.isnan(xo), torch.isnan(ro)), f"{tag}: entry {i} O NaN pattern differs from fp64 math"
        n_nan += int(torch.isnan(rl).sum())
        nan_row = torch.isnan(rl).t()                                              # (sq, h)
        same = (ro == ro_c).all(-1) & (rl == rl_c).t()                             # rows the bad value does not reach
        wave_mate = torch.zeros_like(same)
        if case == "k_inf":
            # a +inf score raises the running max of its whole 32-row wave (the refresh is one ballot per wave): rows that share a wave with such
            # a row but cannot see the key take the refresh path too, which is exact up to the rounding of P (the contract's weaker statement)
            n32 = -(-lq[i] // 32) * 32
            blk = torch.zeros(n32, nan_row.shape[1], dtype=torch.bool, device=gpu)
            blk[:lq[i]] = nan_row
            wave_mate = blk.view(-1, 32, blk.shape[1]).any(1, keepdim=True).expand(-1, 32, -1).reshape(n32, -1)[:lq[i]] & same
        keep = same & ~wave_mate
        assert torch.equal(U.bits(xo[keep]), U.bits(co[keep])) and torch.equal(U.bits(xl.t()[keep]), U.bits(cl.t()[keep])), \
            f"{tag}: entry {i}: a row that cannot see the bad value changed"
        lost = (~same & ~nan_row) | wave_mate                                      # a -inf score: the key drops out; or a wave mate of a +inf row
        n_lost += int(lost.sum())
        if lost.any():
            U.assert_close(xo[lost].float().cpu().numpy(), ro[lost].cpu().numpy(), dtype, f"O {tag} entry {i} rows that lost a key")
            assert (xl.t()[lost].double() - rl.t()[lost]).abs().max().item() <= U.LSE_TOL, tag
        dead = (rl == 0).t() & (ro == 0).all(-1)
        assert (xo[dead] == 0).all().item() and (xl.t()[dead] == 0).all().item(), f"{tag}: entry {i}: a dead row is not O = 0, LSE = 0"
        if causal and layout == "packed" and i == 1:
            assert dead[:30].all().item(), "the short neighbour's first rows must see no key"
    assert n_nan > 0, "the case must produce NaN rows"
    if case == "k_inf":
        assert n_lost > 0, "a +inf K element must drop its key from the rows whose query component is negative"


# ---- C + E. memory outside the problem: never read, never written --------------------------------------------------------------------

def _guard_ok(buf, before, sl):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[sl] = True
    return torch.equal(U.bits(buf)[~inside], before[~inside])


def _workspace(p, split, dev):
    """a NaN-prefilled workspace followed by 64 sentinel floats (split) or none; returns (workspace, whole buffer)"""
    if not split:
        return None, None
    need = capi.bwd_workspace_bytes(p)
    assert need > 0, "the launch must split its head groups through the workspace"
    buf = _s32(need // 4 + 64, dev)
    buf[:need // 4] = float("nan")
    p.workspace, p.workspace_bytes = buf.data_ptr(), need
    return buf[:need // 4], buf


def _dense_capi(q, k, v, do, causal, split, outs):
    """forward + backward through the C ABI into the given output views; returns the workspace buffer"""
    o, lse, dq, dk, dv, dsum = outs
    capi.run_fwd(capi.fwd_params(q, k, v, o, lse, causal))
    p = capi.bwd_params(q, k, v, o, lse, do, dq, dk, dv, dsum, causal)
    _, wbuf = _workspace(p, split, q.device)
    capi.run_bwd(p)
    torch.cuda.synchronize()
    return p, wbuf


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_dense_views_in_poison_and_sentinel_bands(gpu, d, causal, split, pinned_set):
    """Q, K, V, O and dO are views into buffers of NaN, +-inf and 65504 with gaps between rows (pitch >= d + 8), between heads (K: every
    other head of its buffer), between batch entries and after each entry's last row; O, dQ, dK, dV are views into sentinel buffers,
    LSE and dsoftmax_sum sit inside larger ones, the workspace is followed by guard floats.  Through the host module and through the
    C ABI (the whole backward and its three stages one by one): every output is bit-identical to the same call on clean contiguous
    copies, every byte outside the outputs keeps its sentinel, every element inside them is written."""
    dt = torch.float16 if d == 128 else torch.bfloat16
    b, sq, sk, h, hk = 2, 300, 555, 4, 2
    gen = torch.Generator(device=gpu).manual_seed(5000 + d + int(causal))
    q, k, v, do = _rand((b, sq, h, d), dt, gen, gpu), _rand((b, sk, hk, d), dt, gen, gpu), _rand((b, sk, hk, d), dt, gen, gpu), _rand((b, sq, h, d), dt, gen, gpu)
    # clean contiguous reference, C ABI
    ref = (torch.empty_like(q), torch.empty(b, h, sq, device=gpu), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty(b, h, sq, device=gpu))
    _dense_capi(q, k, v, do, causal, split, ref)
    # poisoned inputs
    def poisoned(t, pad):
        _, view, _ = U.guarded(tuple(t.shape), dt, gpu, pad, fill=None)
        view.copy_(t)
        return view
    qp, vp, dop = poisoned(q, (1, 5, 2, 16)), poisoned(v, (2, 3, 1, 24)), poisoned(do, (1, 4, 3, 16))
    kbuf = U.poison_(torch.empty(b + 1, sk + 7, 2 * hk + 1, d + 16, dtype=dt, device=gpu))
    kp = kbuf[1:, 3:3 + sk, 1::2, 8:8 + d]                          # every other head of its buffer
    kp.copy_(k)
    for t in (qp, kp, vp, dop):
        assert all(s % 8 == 0 for s in t.stride()[:3]) and t.stride(1) >= t.shape[-1] + 8, t.stride()
    # host module
    o_h, l_h = F.fwd(q, k, v, causal)
    o_hp, l_hp = F.fwd(qp, kp, vp, causal)
    assert _same(o_hp, o_h) and _same(l_hp, l_h), "host module forward read outside its views"
    op = poisoned(o_h, (1, 2, 2, 16))
    g_h = F.bwd(q, k, v, o_h, l_h, do, causal)
    g_hp = F.bwd(qp, kp, vp, op, l_hp, dop, causal)
    for name, x, r in zip(("dQ", "dK", "dV"), g_hp, g_h):
        assert _same(x, r), f"host module backward: {name} read outside its views"
    # C ABI: sentinel-banded outputs
    bufs = [U.guarded(s, dt, gpu, pad) for s, pad in (((b, sq, h, d), (1, 2, 3, 16)), ((b, sq, h, d), (2, 3, 1, 16)),
                                                    ((b, sk, hk, d), (1, 4, 2, 24)), ((b, sk, hk, d), (2, 1, 2, 16)))]
    lbuf, dbuf = _s32(b * h * sq + 128, gpu), _s32(b * h * sq + 128, gpu)
    before = [U.bits(x[0]).clone() for x in bufs] + [U.bits(lbuf).clone(), U.bits(dbuf).clone()]
    lse, dsum = lbuf[64:64 + b * h * sq].view(b, h, sq), dbuf[64:64 + b * h * sq].view(b, h, sq)
    outs = (bufs[0][1], lse, bufs[1][1], bufs[2][1], bufs[3][1], dsum)
    p, wbuf = _dense_capi(qp, kp, vp, dop, causal, split, outs)
    tag = f"d{d} causal={causal} split={split} {pinned_set}"
    for name, x, r in zip(("O", "LSE", "dQ", "dK", "dV", "dsoftmax_sum"), outs, ref):
        assert _same(x, r), f"C ABI {name} differs from the clean contiguous run [{tag}]"
    for name, (buf, _, sl), b0 in zip(("O", "dQ", "dK", "dV"), bufs, before):
        assert _guard_ok(buf, b0, sl), f"C ABI: bytes outside the {name} view written [{tag}]"
    for name, buf, b0 in (("LSE", lbuf, before[4]), ("dsoftmax_sum", dbuf, before[5])):
        n = b * h * sq
        assert torch.equal(U.bits(buf)[:64], b0[:64]) and torch.equal(U.bits(buf)[64 + n:], b0[64 + n:]), f"{name} guard written [{tag}]"
    if wbuf is not None:
        assert (U.bits(wbuf)[-64:] == SENT32).all().item(), f"workspace guard written [{tag}]"
    # the three backward stages one by one, into fresh sentinel outputs
    for _, x, _ in bufs[1:]:
        x.view(torch.int16).fill_(U.SENT16)
    dsum.view(torch.int32).fill_(SENT32)
    if wbuf is not None:
        wbuf[:-64] = float("nan")
    for stage in ("dot_do_o", "dq", "dkdv"):
        capi.bwd_stage(stage, p)
    torch.cuda.synchronize()
    for name, x, r in zip(("dQ", "dK", "dV", "dsoftmax_sum"), outs[2:], ref[2:]):
        assert _same(x, r), f"stage by stage: {name} differs [{tag}]"
    for name, (buf, _, sl), b0 in zip(("dQ", "dK", "dV"), bufs[1:], before[1:4]):
        assert _guard_ok(buf, b0, sl), f"stage by stage: bytes outside the {name} view written [{tag}]"
    if wbuf is not None:
        assert (U.bits(wbuf)[-64:] == SENT32).all().item(), f"stage by stage: workspace guard written [{tag}]"


def _packed_params(q, k, v, o, lse, do, dq, dk, dv, dsum, cu_q, cu_k, b, mq, mk, causal, total_q, total_k):
    row = lambda t: capi.Strides(0, t.stride(0), t.stride(1))
    h, hk, d = q.shape[1], k.shape[1], q.shape[2]
    common = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(), cu_seqlens_q=cu_q.data_ptr(), cu_seqlens_k=cu_k.data_ptr(),
                  b=b, seqlen_q=mq, seqlen_k=mk, h=h, h_k=hk, d=d, dtype=capi.dtype_code(q.dtype), is_causal=int(causal),
                  q_stride=row(q), k_stride=row(k), v_stride=row(v), o_stride=row(o), total_q=total_q, total_k=total_k)
    fp = capi.FwdParams(**common)
    bp = capi.BwdParams(dout=do.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), dsoftmax_sum=dsum.data_ptr(),
                        do_stride=row(do), dq_stride=row(dq), dk_stride=row(dk), dv_stride=row(dv), **common)
    return fp, bp


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_packed_padding_is_never_read_or_written(gpu, d, causal, split, pinned_set):
    """Packed sequences through the C ABI, total_q / total_k covering 64 padding rows past cu_seqlens[-1]: those rows of q, k, v and
    dout hold NaN, +-inf and 65504 (and the heads' gaps as well); between the forward and the backward the padded LSE entries and the
    dsoftmax_sum entries of rows at or past each sequence's length are poisoned too.  O, LSE, dQ, dK and dV equal the clean contiguous
    call's bits; the padding rows of O, dQ, dK, dV, the padded LSE entries and everything around the outputs keep their sentinel."""
    dt = torch.float16 if d == 128 else torch.bfloat16
    h, hk, pad = 8, 2, 64
    lq, lk = [300, 1, 517, 129, 70], [300, 40, 517, 200, 20]
    b, mq, mk = len(lq), max(lq), max(lk)
    tq, tk = sum(lq) + pad, sum(lk) + pad
    cu_q = torch.tensor(np.concatenate([[0], np.cumsum(lq)]).astype(np.int32), device=gpu)
    cu_k = torch.tensor(np.concatenate([[0], np.cumsum(lk)]).astype(np.int32), device=gpu)
    gen = torch.Generator(device=gpu).manual_seed(6000 + d + int(causal))
    q, do = _rand((tq, h, d), dt, gen, gpu), _rand((tq, h, d), dt, gen, gpu)
    k, v = _rand((tk, hk, d), dt, gen, gpu), _rand((tk, hk, d), dt, gen, gpu)
    for t, n in ((q, sum(lq)), (do, sum(lq)), (k, sum(lk)), (v, sum(lk))):
        t[n:] = 0
    tag = f"d{d} causal={causal} split={split} {pinned_set}"

    def run(qq, kk, vv, dd, outs, poison_between):
        o, lse, dq, dk, dv, dsum = outs
        fp, bp = _packed_params(qq, kk, vv, o, lse, dd, dq, dk, dv, dsum, cu_q, cu_k, b, mq, mk, causal, tq, tk)
        capi.run_fwd(fp)
        torch.cuda.synchronize()
        if poison_between:
            for i, n in enumerate(lq):
                assert (U.bits(lse[i, :, n:]) == SENT32).all().item(), f"padded LSE entries of sequence {i} written [{tag}]"
                U.poison_(lse[i, :, n:])
                U.poison_(dsum[i, :, n:])
        _, wbuf = _workspace(bp, split, qq.device)
        capi.run_bwd(bp)
        torch.cuda.synchronize()
        return wbuf

    ref = (torch.zeros_like(q), torch.zeros(b, h, mq, device=gpu), torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v), torch.zeros(b, h, mq, device=gpu))
    run(q, k, v, do, ref, False)

    def poisoned(t, n, hpad):
        _, view, _ = U.guarded(tuple(t.shape), dt, gpu, (0, hpad, 16), fill=None)
        view[:n] = t[:n]
        return view

    qp, dop, kp, vp = poisoned(q, sum(lq), 2), poisoned(do, sum(lq), 1), poisoned(k, sum(lk), 3), poisoned(v, sum(lk), 2)
    bufs = [U.guarded(s, dt, gpu, pd) for s, pd in (((tq, h, d), (4, 2, 16)), ((tq, h, d), (2, 1, 16)), ((tk, hk, d), (6, 2, 24)), ((tk, hk, d), (2, 3, 16)))]
    lbuf, dbuf = _s32(b * h * mq + 128, gpu), _s32(b * h * mq + 128, gpu)
    before = [U.bits(x[0]).clone() for x in bufs]
    lse, dsum = lbuf[64:64 + b * h * mq].view(b, h, mq), dbuf[64:64 + b * h * mq].view(b, h, mq)
    outs = (bufs[0][1], lse, bufs[1][1], bufs[2][1], bufs[3][1], dsum)
    lb0, db0 = U.bits(lbuf).clone(), U.bits(dbuf).clone()
    wbuf = run(qp, kp, vp, dop, outs, True)
    n = b * h * mq
    for name, buf, b0 in (("LSE", lbuf, lb0), ("dsoftmax_sum", dbuf, db0)):
        assert torch.equal(U.bits(buf)[:64], b0[:64]) and torch.equal(U.bits(buf)[64 + n:], b0[64 + n:]), f"{name} guard written [{tag}]"
    if wbuf is not None:
        assert (U.bits(wbuf)[-64:] == SENT32).all().item(), f"workspace guard written [{tag}]"
    for name, (buf, x, sl), b0, r, tot in zip(("O", "dQ", "dK", "dV"), bufs, before, (ref[0], ref[2], ref[3], ref[4]), (sum(lq), sum(lq), sum(lk), sum(lk))):
        assert _guard_ok(buf, b0, sl), f"bytes outside the {name} view written [{tag}]"
        assert (U.bits(x[tot:]) == U.SENT16).all().item(), f"{name}: padding rows past cu_seqlens[-1] written [{tag}]"
        assert _same(x[:tot], r[:tot]), f"{name} differs from the clean contiguous call [{tag}]"
    for i, m in enumerate(lq):
        assert _same(lse[i, :, :m], ref[1][i, :, :m]), f"LSE of sequence {i} differs [{tag}]"


# ---- D. items are isolated -----------------------------------------------------------------------------------------------------------

def _dense_all(q, k, v, do, causal, split):
    outs = (torch.empty_like(q), torch.empty(q.shape[0], q.shape[2], q.shape[1], device=q.device), torch.empty_like(q), torch.empty_like(k),
            torch.empty_like(v), torch.empty(q.shape[0], q.shape[2], q.shape[1], device=q.device))
    _dense_capi(q, k, v, do, causal, split, outs)
    return outs[:5]


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_nan_item_leaves_the_other_items_bits(gpu, d, causal, split, pinned_set):
    """One whole item filled with NaN, everything else clean: every other item's O, LSE, dQ, dK and dV are bit-identical to the clean
    run.  Items: a batch entry; a KV head with its query heads; a query head alone (its group's dK / dV go NaN, every other head's
    O, LSE, dQ and every other group's dK / dV keep their bits); a packed sequence next to a ragged neighbour on the plain grid
    (total = 0) and on the compact grid (under a causal mask with 8 heads and at most 64 sequences: the heavy-first lookup)."""
    dt = torch.float16 if d == 128 else torch.bfloat16
    b, sq, sk, h, hk = 3, 300, 555, 8, 2
    r = h // hk
    gen = torch.Generator(device=gpu).manual_seed(7000 + d + int(causal))
    q, do = _rand((b, sq, h, d), dt, gen, gpu), _rand((b, sq, h, d), dt, gen, gpu)
    k, v = _rand((b, sk, hk, d), dt, gen, gpu), _rand((b, sk, hk, d), dt, gen, gpu)
    clean = _dense_all(q, k, v, do, causal, split)
    tag = f"d{d} causal={causal} split={split} {pinned_set}"
    names = ("O", "LSE", "dQ", "dK", "dV")
    # (item, q/dO index, k/v index, kept q-side index, kept k-side index); LSE is (b, h, sq)
    items = (("batch entry 1", (1,), (1,), ([0, 2],), ([0, 2],)),
             ("kv head 1 + its query heads", (slice(None), slice(None), slice(r, 2 * r)), (slice(None), slice(None), 1),
              (slice(None), slice(None), [i for i in range(h) if not r <= i < 2 * r]), (slice(None), slice(None), 0)),
             ("query head 5 alone", (slice(None), slice(None), 5), None,
              (slice(None), slice(None), [i for i in range(h) if i != 5]), (slice(None), slice(None), [g for g in range(hk) if g != 5 // r])))
    for name, qi, ki, keep_q, keep_k in items:
        qn, kn, vn, don = q.clone(), k.clone(), v.clone(), do.clone()
        qn[qi], don[qi] = float("nan"), float("nan")
        if ki is not None:
            kn[ki], vn[ki] = float("nan"), float("nan")
        got = _dense_all(qn, kn, vn, don, causal, split)
        lse_keep = (keep_q[0],) if len(keep_q) == 1 else (slice(None), keep_q[2])
        for nm, x, c in zip(names, got, clean):
            idx = lse_keep if nm == "LSE" else (keep_k if nm in ("dK", "dV") else keep_q)
            assert _same(x[idx], c[idx]), f"{name}: {nm} of another item changed [{tag}]"
            assert torch.isnan(x).any().item(), f"{name}: the NaN item must reach {nm}"
    # packed: sequence 2 of 5 (a ragged neighbour on each side) on both grids
    lq, lk = [300, 129, 517, 1, 70], [555, 200, 517, 40, 20]
    tq, tk = sum(lq), sum(lk)
    cu_q = torch.tensor(np.concatenate([[0], np.cumsum(lq)]).astype(np.int32), device=gpu)
    cu_k = torch.tensor(np.concatenate([[0], np.cumsum(lk)]).astype(np.int32), device=gpu)
    qv, dov = _rand((tq, h, d), dt, gen, gpu), _rand((tq, h, d), dt, gen, gpu)
    kv, vv = _rand((tk, hk, d), dt, gen, gpu), _rand((tk, hk, d), dt, gen, gpu)
    nb, mq, mk = len(lq), max(lq), max(lk)
    a_q, e_q, a_k, e_k = int(cu_q[2]), int(cu_q[3]), int(cu_k[2]), int(cu_k[3])

    def packed(qq, kk, vv_, dd, total):
        outs = (torch.zeros_like(qq), torch.zeros(nb, h, mq, device=gpu), torch.zeros_like(qq), torch.zeros_like(kk), torch.zeros_like(vv_), torch.zeros(nb, h, mq, device=gpu))
        fp, bp = _packed_params(qq, kk, vv_, outs[0], outs[1], dd, outs[2], outs[3], outs[4], outs[5], cu_q, cu_k, nb, mq, mk, causal,
                                tq if total else 0, tk if total else 0)
        capi.run_fwd(fp)
        ws = _workspace(bp, split and total, gpu)
        capi.run_bwd(bp)
        torch.cuda.synchronize()
        del ws
        return outs[:5]

    for total in (False, True):
        cl = packed(qv, kv, vv, dov, total)
        qn, kn, vn, don = qv.clone(), kv.clone(), vv.clone(), dov.clone()
        qn[a_q:e_q], don[a_q:e_q], kn[a_k:e_k], vn[a_k:e_k] = (float("nan"),) * 4
        got = packed(qn, kn, vn, don, total)
        keep_q = torch.ones(tq, dtype=torch.bool, device=gpu); keep_q[a_q:e_q] = False
        keep_k = torch.ones(tk, dtype=torch.bool, device=gpu); keep_k[a_k:e_k] = False
        grid = ("compact grid, heavy-first lookup" if causal else "compact grid") if total else "plain grid"
        for nm, x, c in zip(names, got, cl):
            if nm == "LSE":
                x, c = torch.cat([x[:2], x[3:]]), torch.cat([c[:2], c[3:]])
            else:
                x, c = (x[keep_k], c[keep_k]) if nm in ("dK", "dV") else (x[keep_q], c[keep_q])
            assert _same(x, c), f"packed sequence 2 ({grid}): {nm} of another sequence changed [{tag}]"
