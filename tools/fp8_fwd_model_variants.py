#!/usr/bin/env python3
"""CPU: the rounding model of tests/test_fp8_fwd_gpu.py against three neighbours of the quantisation contract - P = e4m3(p) without the x 256, 256 p truncated
instead of rounded, the denominator summed over the rounded P - on the test's own inputs: which of them the 1.25 budget separates, and which the tail case
does (the line of DESIGN.md 3.25)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "flash-attention-turing_amd")]      # (the test module imports the built package)
import test_fp8_fwd_gpu as T
E4M3 = T.E4M3
def trunc8(x):   # e4m3 truncation toward zero of non-negative fp32
    r = x.float().to(E4M3).float()
    up = r > x.float()
    b = r.to(E4M3).view(torch.uint8)
    return torch.where(up, (b - 1).view(E4M3).float(), r).double()
def variant(qc, kc, vc, qd, kd, vd, causal, kind):
    (sq, h), (sk, hk) = qc.shape[:2], kc.shape[:2]
    q = qc.double() * qd[0, :, None].double()
    k = (kc.double() * kd[0, :, None].double()).repeat_interleave(h // hk, 1)
    v = (vc.double() * vd[0, :, None].double()).repeat_interleave(h // hk, 1)
    s = torch.einsum("thd,jhd->htj", q, k) * T.SCALE
    t, j = torch.arange(sq)[:, None], torch.arange(sk)[None, :]
    s = s.masked_fill(~((j <= sk - sq + t) if causal else torch.ones(sq, sk, dtype=torch.bool)), float("-inf"))
    m, l, acc = torch.full((h, sq), -1e30, dtype=torch.float64), torch.zeros(h, sq, dtype=torch.float64), torch.zeros(sq, h, 128, dtype=torch.float64)
    for j0 in range(0, sk, 128):
        m_new = torch.maximum(m, s[..., j0:j0 + 128].amax(-1))
        p, alpha = torch.exp(s[..., j0:j0 + 128] - m_new[..., None]), torch.exp(m - m_new)
        if kind == "no256": p8 = p.float().to(E4M3).double()
        elif kind == "trunc": p8 = trunc8(256 * p) / 256
        else: p8 = (256 * p).float().to(E4M3).double() / 256
        ps = p8 if kind == "lrounded" else p
        l, acc, m = l * alpha + ps.sum(-1), acc * alpha.T[..., None] + torch.einsum("htj,jhd->thd", p8, v[j0:j0 + 128]), m_new
    return acc / l.T.clamp_min(1e-300)[..., None], m + torch.log(l.clamp_min(1e-300))
R = {k: [] for k in ("no256", "trunc", "lrounded")}
for dt in ("bf16", "fp16"):
  for causal in (False, True):
    for h, hk in ((2, 2), (4, 1)):
      for n, (sq, sk) in enumerate(T.SHAPES):
        ins = T._inputs(sq, sk, h, hk, 7000 + n)
        o64, l64, model, dead = T._model(*ins, causal)
        if dead.all() or sk == 1: continue
        em = T._relrms(model.to(T.DT[dt]).double(), o64)
        for kind in R:
            o, _ = variant(*ins, causal, kind)
            R[kind].append(T._relrms(o.to(T.DT[dt]).double(), o64) / em)
for k, v in R.items(): print("random cases", k, "ratio to model %.4f .. %.4f" % (min(v), max(v)))
q, k, v = (torch.zeros(n, 1, 128) for n in (1, 2001, 2001))
q[0, 0, 0], k[0, 0, 0] = 8.0, 16.0
v[1:, 0] = (torch.arange(128) % 7 + 1).float()
ins = (q.to(E4M3), k.to(E4M3), v.to(E4M3), torch.ones(1, 1), torch.ones(1, 1), torch.tensor([[0.37]]))
_, l64, model, _ = T._model(*ins, False)
print("tail case: model rounded to fp16 rel err %.3e" % float(((model.half().double() - model) / model).abs().max()))
for kind in R:
    o, l = variant(*ins, False, kind)
    print("tail case", kind, "out max rel err %.3e  lse err %.3e" % (float(((o - model) / model).abs().max()), float((l.T - l64.T).abs().max())))
