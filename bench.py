#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X attention path (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one forward pass of the hot path (C ABI `fa_mha_fwd`, include/flash_attn_gfx950.h)
over one batch of synthetic N(0,1) inputs that are already resident in HBM.  Workload at every N:
BASELINE.json configs[2] per GPU — forward, b=4, seq=16384, h=32, d=128, fp16, causal — the
configuration the metric ("attention fwd TFLOP/s & % MFMA peak, b4 h32 d128 seq16k") is quoted
on.  Multi-GPU is weak scaling over independent (batch, head) problems: every rank owns its own
b=4 shard (N=8 is BASELINE configs[4]'s b=32), no data-path collective; the only
communication is the timing barrier and a MAX all-reduce of the elapsed time.

Prints ONE JSON line on rank 0: `value` = whole-job TFLOP/s using the ALGORITHMIC FLOPs of
SURVEY.md §8(d) (4*b*h*sq*sk*d, x1/2 causal), `ms_per_step` = wall milliseconds of one timed step.
A plain run does nothing else: set-up, W warm-up steps, K timed steps, the line.  `--dump-outputs DIR`
writes what the last timed step computed as DIR/<name>.npy (dump_outputs).  With `--full` the line also carries
`roofline` for the dominant kernel (the forward kernel) from HIP-event timing on the launch stream,
`cpu_baseline` = the CPU oracle (oracle/, the checker, never the product) timed on a bounded
sample on rank 0 at N=1, plus PyTorch SDPA's CPU math path at BASELINE configs[0] as the
north_star asks.  `extra` carries, after the timed region:
  N = 1: the other BASELINE configs (with `roofline_bwd` for the three backward kernels of configs[3]) and the reference
         README's seqlen sweep 512..16k (b4 h32 d128 fp16) next to PyTorch-ROCm SDPA on the same GPU;
  N > 1: the same seqlen sweep STRONG-scaled over the N ranks (the b=4 x h=32 problem split by `plan_shards`: batch slices at
         N = 2 / 4, batch x kv-head halves at N = 8, strided views, no copy, no collective) with per-point aggregate TFLOP/s and
         efficiency against rank 0 running the whole problem alone in the same run, and BASELINE configs[4] itself
         (non-causal 16k, b=4 per rank = b=32 at N=8) as a weak-scaled line.

Communication: the timing harness needs a barrier and a scalar MAX, nothing else.  The default process group is gloo (cannot
fail for want of a GPU fabric); with `--backend nccl` (default) an nccl (= RCCL) group is created on top and used for the
barrier / reductions if — and only if — every rank could create it and complete a device all-reduce; otherwise the harness
stays on gloo and says so in the JSON (`comm_backend`).
"""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-turing_amd"))
sys.path.insert(0, ROOT)

PEAK_DENSE_FP16_TFLOPS = 2500.0   # MI355X dense fp16/bf16 MFMA peak (MI355X_MICROARCH.md: ~2.5 PF dense)
PEAK_HBM_GBPS = 8000.0
MFMA_FLOP_PER_CLK_PER_CU = 4096   # 4 SIMDs x (32x32x16 MFMA = 32768 FLOP / 32 clk)
SWEEP_SEQS = (512, 1024, 2048, 4096, 8192, 16384)   # reference benchmark.sh:17-21 (power-of-two half), README.md:7-16

WORKLOADS = {
    # name: (b, seq, h, h_k, d, dtype, causal, backward)
    "c3": (4, 16384, 32, 32, 128, "fp16", True, False),    # BASELINE configs[2]  (headline)
    "c2": (4, 4096, 32, 32, 128, "fp16", False, False),    # BASELINE configs[1]
    "c4": (4, 8192, 32, 32, 128, "bf16", False, True),     # BASELINE configs[3]  fwd+bwd
    "c5shard": (4, 16384, 32, 32, 128, "fp16", False, False),  # one GPU's share of configs[4]
}


def fwd_flops(b, sq, sk, h, d, causal):
    """4*b*h*sq*sk*d, halved for causal (sq == sk)."""
    f = 4.0 * b * h * sq * sk * d
    return f * 0.5 if causal else f


def fwd_bytes(b, sq, sk, h, hk, d):
    return 2.0 * (b * sq * h * d * 2.0) + 2.0 * (b * sk * hk * d * 2.0) + b * h * sq * 4.0


class Dist:
    """Minimal one-process-per-GPU harness: env-driven init, barrier, MAX / SUM / MIN reductions.

    Default group: gloo (CPU tensors).  `want` == "nccl": an nccl (= RCCL) group is added with new_group() and adopted for
    barrier / reductions only if all ranks created it and finished one device all-reduce (agreement by a gloo MIN);
    any failure leaves the harness on gloo with the reason recorded in `comm_backend`."""

    def __init__(self, want):
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.want = want
        self.group = None          # None = default (gloo) group
        self.on_device = False
        # the backend of the subgroup `want == "nccl"` asks for.  FA_BENCH_SUBGROUP_BACKEND=gloo stands a CPU process group in for RCCL so
        # that the SUCCESS branch of the adoption (every rank initialised -> subgroup adopted -> barrier and reductions go through it) can
        # be driven without GPUs (tests/test_dist_cpu.py); the subgroup's tensors then live on the CPU.
        self.sub_backend = os.environ.get("FA_BENCH_SUBGROUP_BACKEND", "nccl")
        self.sub_calls = {"barrier": 0, "all_reduce": 0}      # collectives that went through the adopted subgroup
        self.comm_backend = "none (single process)"
        # FA_BENCH_FORCE_PG=1: create the process groups even at world size 1, so that the real init / barrier / all_reduce
        # calls of the N > 1 path can be exercised on a 1-GPU box (RCCL refuses two ranks on one device)
        self.enabled = self.world > 1 or os.environ.get("FA_BENCH_FORCE_PG") == "1"
        if self.enabled:
            import torch.distributed as dist

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29500")
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            dist.init_process_group(backend="gloo", rank=self.rank, world_size=self.world,
                                    timeout=datetime.timedelta(seconds=600))
            self.dist = dist
            self.comm_backend = "gloo"

    def try_nccl(self, device):
        """called once the rank's device is set; returns the adopted backend string"""
        if not self.enabled or self.want != "nccl":
            return self.comm_backend
        import torch

        ok, why = 1.0, ""
        grp = None
        on_gpu = self.sub_backend == "nccl"
        try:
            grp = self.dist.new_group(backend=self.sub_backend, timeout=datetime.timedelta(seconds=180))
            t = torch.ones(1, dtype=torch.float64, device=device if on_gpu else "cpu")
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=grp)
            if on_gpu:
                torch.cuda.synchronize(device)
            if int(t.item()) != self.world:
                ok, why = 0.0, f"nccl all_reduce returned {t.item()} for world {self.world}"
        except Exception as e:  # noqa: BLE001 - reported in the JSON, the harness continues on gloo
            ok, why = 0.0, f"{type(e).__name__}: {str(e)[:160]}"
        agree = torch.tensor([ok], dtype=torch.float64)
        self.dist.all_reduce(agree, op=self.dist.ReduceOp.MIN)      # default (gloo) group: every rank learns the verdict
        if agree.item() >= 1.0:
            self.group, self.on_device = grp, on_gpu
            self.comm_backend = "nccl (RCCL)" if on_gpu else f"{self.sub_backend} subgroup standing in for nccl (FA_BENCH_SUBGROUP_BACKEND)"
        else:
            self.comm_backend = "gloo (nccl unavailable" + (f": {why}" if why else " on another rank") + ")"
        return self.comm_backend

    def _tensor(self, x, device):
        import torch

        return torch.tensor([x], dtype=torch.float64, device=device if self.on_device else "cpu")

    def barrier(self, device=None):
        if not self.enabled:
            return
        if self.group is not None:
            self.sub_calls["barrier"] += 1
        if self.on_device:
            self.dist.barrier(group=self.group, device_ids=[device.index if device is not None else self.local_rank])
        else:
            self.dist.barrier(group=self.group)

    def _reduce(self, x, op, device):
        if not self.enabled:
            return x
        t = self._tensor(x, device)
        if self.group is not None:
            self.sub_calls["all_reduce"] += 1
        self.dist.all_reduce(t, op=op, group=self.group)
        return float(t.item())

    def reduce_max(self, x, device=None):
        return self._reduce(x, self.dist.ReduceOp.MAX, device) if self.enabled else x

    def reduce_sum(self, x, device=None):
        return self._reduce(x, self.dist.ReduceOp.SUM, device) if self.enabled else x

    def close(self):
        if self.enabled:
            self.dist.destroy_process_group()


def timed_region(step_fn, steps, warmup, dist, sync_fn, device=None, events=None):
    """W untimed warm-up steps, then exactly K steps bracketed by barrier + device sync on both
    sides; returns (max-over-ranks wall seconds for the K steps, local wall seconds).  `events` = (start, end) HIP events recorded on the
    launch stream directly around the K steps: the device-side duration of the SAME launches the wall clock brackets (roofline.achieved)."""
    for _ in range(warmup):
        step_fn()
    sync_fn()
    dist.barrier(device)
    sync_fn()
    t0 = time.perf_counter()
    if events is not None:
        events[0].record()
    for _ in range(steps):
        step_fn()
    if events is not None:
        events[1].record()
    sync_fn()
    dist.barrier(device)
    sync_fn()
    local = time.perf_counter() - t0
    return dist.reduce_max(local, device), local


def strong_scaling_sweep(dist, make_point, sync_fn, device, seqs=SWEEP_SEQS, causals=(False, True), b=4, h=32, hk=32, d=128):
    """The README seqlen sweep of ONE b x h problem split over the ranks by plan_shards (batch slices, then kv-head groups).

    make_point(seq, causal, plan) -> (step_shard, step_whole): callables running this rank's shard / the whole problem once.
    Per point: rank 0 alone times the whole problem (the in-run N = 1 reference), then all ranks time their shards between
    barriers; aggregate TFLOP/s = whole-problem FLOPs / MAX-over-ranks time; efficiency = aggregate / (N x single-GPU rate)."""
    from flash_attn_turing.sharding import plan_shards, problem_policy

    plan = plan_shards(b, h, hk, dist.world)[dist.rank]
    out = {}
    for causal in causals:
        for seq in seqs:
            step_shard_own, step_whole = make_point(seq, causal, plan)

            def step_shard(f=step_shard_own):
                # the shard is served by the kernels the WHOLE problem gets (FA_POLICY_AUTO sizes a launch by its workgroups; a shard states the whole problem's
                # batch x heads): its results are bit-identical to the unsharded call's, tests/test_properties_gpu.py
                with problem_policy(b, h):
                    f()
            iters = 20      # (round 6: also at 8k / 16k, where 6 launches were a 40 ms window - shorter than the clock's settling time, 1-3 % optimistic against the headline's 20)
            flops = fwd_flops(b, seq, seq, h, d, causal)
            single = None
            if dist.rank == 0:
                t1, _ = timed_region(step_whole, iters, 2, _NoDist, sync_fn, device)
                single = flops * iters / t1 / 1e12
            dist.barrier(device)
            wall, local = timed_region(step_shard, iters, 2, dist, sync_fn, device)
            agg = flops * iters / wall / 1e12
            units = dist.reduce_sum(float(plan.n_units), device)
            if dist.rank == 0:
                out[f"{seq}{'_causal' if causal else ''}"] = {
                    "seq": seq, "causal": causal, "ms": wall / iters * 1e3, "aggregate_tflops": agg,
                    "frac_of_fp16_mfma_peak": agg / (PEAK_DENSE_FP16_TFLOPS * dist.world),
                    "single_gpu_tflops_same_run": single, "efficiency_vs_1gpu": agg / (single * dist.world),
                    "units_total": units, "shard_kernel_policy": "whole problem's (flash_attn_turing.sharding.problem_policy)",
                    "shard": f"batch [{plan.batch_start},{plan.batch_stop}) x kv heads [{plan.head_k_start},{plan.head_k_stop}) on rank 0"}
    return out


class _NoDistT:
    """stand-in for Dist when only one rank times something alone"""

    def barrier(self, device=None):
        pass

    def reduce_max(self, x, device=None):
        return x


_NoDist = _NoDistT()


def make_inputs(torch, device, b, s, h, hk, d, dtype, seed, backward):
    gen = torch.Generator(device=device).manual_seed(seed)
    tdt = torch.float16 if dtype == "fp16" else torch.bfloat16
    q = torch.randn(b, s, h, d, device=device, dtype=tdt, generator=gen)
    k = torch.randn(b, s, hk, d, device=device, dtype=tdt, generator=gen)
    v = torch.randn(b, s, hk, d, device=device, dtype=tdt, generator=gen)
    t = dict(q=q, k=k, v=v, o=torch.empty_like(q), lse=torch.empty(b, h, s, device=device, dtype=torch.float32))
    if backward:
        t.update(dout=torch.randn(b, s, h, d, device=device, dtype=tdt, generator=gen), dq=torch.empty_like(q),
                 dk=torch.empty_like(k), dv=torch.empty_like(v), dsum=torch.empty_like(t["lse"]))
    return t


def event_time_ms(torch, fn, iters, reps=1):
    """ms per call, HIP events on torch's current stream (the stream the C ABI launches on): the mean over `iters` back-to-back
    calls; with reps > 1 the MEDIAN of `reps` such means (single 5-call samples of the `extra` configs were seen 5-7 % off on some
    boxes of the pool while the kernels were byte-identical)."""
    import statistics

    means = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        end.synchronize()
        means.append(start.elapsed_time(end) / iters)
    return statistics.median(means)


def launch_time_distribution(torch, fn, n):
    """n individually timed launches (one HIP-event pair each, on the launch stream): mean / median / min / max in ms.
    SURVEY.md 8(d) asks for median AND min over >= 30 iterations; the mean of back-to-back launches (event_time_ms) stays the figure
    `achieved` is computed from, because that is what a rocprofv3 --stats average of the same command reproduces."""
    import statistics

    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    evs[-1][1].synchronize()
    ts = [a.elapsed_time(b) for a, b in evs]
    return {"n": n, "mean_ms": sum(ts) / n, "median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


class PowerSampler:
    """Polls the GPU's own sensors (amdgpu sysfs: hwmon power1_average / power1_input in microwatts, freq1_input = sclk in Hz) from a
    host thread while a region runs.  Substantiates (or refutes) the "power-limited under MFMA load" reading of the clock
    counters.  Costs a few file reads per 5 ms on one host core; nothing is launched on the GPU."""

    def __init__(self, device_index=0, period_s=0.005):
        import glob
        import threading

        self.period, self.samples, self._stop, self._thr = period_s, [], threading.Event(), None
        self.power_path = self.sclk_path = self.cap_w = None
        # the hwmon node of THIS device: /sys/class/drm/cardN/device is a link to its PCI function; match it against the bus id HIP reports
        # (a container may show other GPUs' cards too, and reading a neighbour's sensors would be worse than reading none)
        self.pci = self._pci_bus_id(device_index)
        cands = []
        for c in sorted(glob.glob("/sys/class/drm/card[0-9]*")):
            try:
                addr = os.path.basename(os.path.realpath(os.path.join(c, "device"))).lower()
            except OSError:
                continue
            if self.pci and addr == self.pci:
                cands = sorted(glob.glob(os.path.join(c, "device", "hwmon", "hwmon*")))
                break
        if cands:
            h = cands[0]
            for f in ("power1_average", "power1_input"):
                if os.path.exists(os.path.join(h, f)):
                    self.power_path = os.path.join(h, f)
                    break
            if os.path.exists(os.path.join(h, "freq1_input")):
                self.sclk_path = os.path.join(h, "freq1_input")
            self.cap_w = (self._read(os.path.join(h, "power1_cap")) or 0.0) / 1e6 or None
        self._threading = threading

    @staticmethod
    def _pci_bus_id(device_index):
        """'0000:bb:dd.f' of HIP device `device_index` (hipDeviceGetPCIBusId through ctypes), lower case; None if unavailable"""
        import ctypes

        try:
            hip = ctypes.CDLL("libamdhip64.so")
            buf = ctypes.create_string_buffer(64)
            if hip.hipDeviceGetPCIBusId(buf, 64, int(device_index)) != 0:
                return None
            return buf.value.decode().lower() or None
        except OSError:
            return None

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except (OSError, ValueError):
            return None

    def _run(self):
        while not self._stop.is_set():
            self.samples.append((time.perf_counter(), self._read(self.power_path) if self.power_path else None,
                                 self._read(self.sclk_path) if self.sclk_path else None))
            time.sleep(self.period)

    def __enter__(self):
        if self.power_path or self.sclk_path:
            self._thr = self._threading.Thread(target=self._run, daemon=True)
            self._thr.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        if self._thr is not None:
            self._thr.join(timeout=1.0)

    def summary(self, t0, t1, what):
        if not (self.power_path or self.sclk_path):
            return {"error": f"no amdgpu hwmon power / sclk sensor visible for this device (PCI {self.pci}) under /sys/class/drm", "region": what}
        inside = [x for x in self.samples if t0 <= x[0] <= t1]
        pw = [x[1] / 1e6 for x in inside if x[1] is not None]
        ck = [x[2] / 1e6 for x in inside if x[2] is not None]
        out = {"region": what, "samples": len(inside), "sensor": self.power_path or self.sclk_path, "pci_bus_id": self.pci, "power_cap_w": self.cap_w,
               "note": "freq1_input is the clock the SMU reports (its target), not the delivered one: the effective clock under MFMA load "
                       "comes from GRBM_GUI_ACTIVE / time in profiles/*shader_pmc_summary.json"}
        if pw:
            out.update(power_w_mean=sum(pw) / len(pw), power_w_max=max(pw))
        if ck:
            out.update(sclk_mhz_mean=sum(ck) / len(ck), sclk_mhz_min=min(ck), sclk_mhz_max=max(ck))
        return out


def build_commit():
    """git commit the tree was built from (tools/gpu.sh leaves it next to the package: .git does not travel to the GPU box); None when
    the file is absent (the library's source digest is the authoritative tie between kernels and profiles)"""
    try:
        with open(os.path.join(ROOT, "flash-attention-turing_amd", "BUILD_COMMIT")) as f:
            return f.read().strip() or None
    except OSError:
        return None


def library_source_digest(capi):
    """`src=<12 hex>` of fa_build_info(): sha256 over kernel sources + headers + flags, stamped in by build.py"""
    import re

    m = re.search(r"src=([0-9a-f]+)", capi.lib().fa_build_info().decode())
    return m.group(1) if m else None


def hbm_traffic_from_profile(workload, kernel):
    """(bytes per launch, source) of the dominant kernel from the newest committed rocprofv3 PMC pass for this workload AND this
    kernel (profiles/rNN_hbm_traffic.json: FETCH_SIZE and WRITE_SIZE collected in separate --pmc runs, FETCH_SIZE doubled as
    MI355X_MICROARCH.md prescribes for gfx950).  PMC collection cannot run inside the timed process, so this is a committed
    per-round value, tagged as such; (None, reason) when no profile of this workload / kernel is committed."""
    import glob

    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")), reverse=True):
        try:
            with open(path) as f:
                d = json.load(f)
            if d.get("workload") == workload and d.get("kernel", "fa_fwd_pp_kernel") == kernel:
                return (float(d["traffic_bytes_per_launch"]), f"committed profile {os.path.basename(path)} (not measured in this run)",
                        d.get("library_source_digest"), d.get("git_commit"))
        except (OSError, ValueError, KeyError):
            pass
    return None, f"no committed PMC profile for workload {workload} / kernel {kernel}", None, None


def parse_clockbench(out):
    """tools/clockbench prints one row per variant: `<label>  <min> <median> <max>` (TFLOP/s over interleaved runs).
    Returns the best MEDIAN among the pure-MFMA rows, or a dict with `error` so that a format drift is visible in the JSON."""
    best, small = None, None
    for line in out.splitlines():
        if not (line.startswith("MFMA only") or line.startswith("16x16x32 MFMA only")):
            continue
        parts = line.split()
        try:
            mn, med, mx = (float(x) for x in parts[-3:])
        except ValueError:
            continue
        row = {"tflops": med, "min": mn, "max": mx, "what": " ".join(parts[:-3])}
        if line.startswith("16x16x32"):
            small = row
        elif best is None or med > best["tflops"]:
            best = row
    if best is None:
        return {"error": "no 'MFMA only' row with min/median/max in clockbench output", "head": out[:200]}
    if small is not None:
        best["mfma_16x16x32"] = small      # the same loop from v_mfma_f32_16x16x32: the shape the head_dim-128 16x16x32 kernels use
    return best


def parse_clockbench_rows(out):
    """every row of tools/clockbench as {label: median TFLOP/s}"""
    rows = {}
    for line in out.splitlines():
        parts = line.split()
        if len(parts) >= 4:
            try:
                rows[" ".join(parts[:-3])] = float(parts[-2])
            except ValueError:
                pass
    return rows


PROBE_MIX_D128 = "16x16x32 mix: 3.1 VALU + 1 KiB LDS (fwd d128 now), 2 w/SIMD"
PROBE_PP_D128 = "16x16x32 ping-pong d128: 68 MFMA + 48 LDS | 95 VALU, 8 waves"
PROBE_MIX_D64 = "16x16x32 mix: 5.2 VALU + 1 KiB LDS (fwd d64), 2 w/SIMD"
PROBE_PP_MFMA_ISSUED, PROBE_PP_MFMA_ALGORITHMIC = 68, 64      # tools/clockbench k_pp16<32, ..>: 2 x 32 fragment MFMAs + 4 row-sum MFMAs per wave and step
PROBE_PP_D64 = "16x16x32 ping-pong d64: 68 MFMA + 48 LDS | 190 VALU, 8 waves"
PROBE_PURE16 = "16x16x32 MFMA only, 2 waves/SIMD"


def ceiling_block(workload, kernel, achieved, clock_rows):
    """`roofline.ceiling`: the distance between `achieved` and the nominal 2.5 PFLOP/s, decomposed in the line itself, every step measured IN THIS RUN with the kernel's
    own MFMA shape (until round 5 the mixed rows were v_mfma_f32_32x32x16 loops beside a 16x16x32 kernel):
      nominal peak  ->  a chip-wide loop of NOTHING BUT this kernel's MFMA instruction on N(0,1) operands (the package power cap)
                    ->  the kernel's own STRUCTURE without its dependencies (tools/clockbench k_pp16: eight waves in two groups one phase apart, matrix phase = 68 MFMAs
                        + 48 LDS fragment reads at prefetch depth 2 whose data are the MFMAs' operands, softmax phase = 95 VALU in the softmax's composition, two
                        barriers per tile; no LDS-DMA, no mask, no data dependence between the phases, no prologue / epilogue)
                    ->  achieved.
    Beside the chain: the same instruction mix as ONE interleaved stream per wave (k_mix16, 3.1 VALU + 1 KiB of LDS reads per 32768 FLOP) - the probe the round-3..5
    statements quoted in its 32x32x16 form - and the timing-only ablation builds of the kernel itself (newest committed profile).  None of them is ever used as `peak`."""
    import glob
    import re

    out = {"what": "decomposition of achieved / peak; measured rates under the power cap, never used as `peak`", "nominal_peak_tflops": PEAK_DENSE_FP16_TFLOPS,
           "shipped_tflops": achieved}
    is16 = "16" in kernel
    own = PROBE_PURE16 if is16 else "MFMA only, 2 waves/SIMD"
    if clock_rows:
        out["pure_mfma_on_n01_operands_tflops"] = {"this_kernels_mfma_shape": clock_rows.get(own), "shape": "v_mfma_f32_16x16x32" if is16 else "v_mfma_f32_32x32x16",
                                                  "v_mfma_f32_32x32x16": clock_rows.get("MFMA only, 2 waves/SIMD"), "v_mfma_f32_16x16x32": clock_rows.get(PROBE_PURE16),
                                                  "source": "tools/clockbench in this run (median of 5 interleaved chip-wide runs, random operands)"}
        out["instruction_mix_probe_tflops"] = {k: v for k, v in clock_rows.items() if "VALU" in k or "LDS" in k}
        out["instruction_mix_probe_note"] = ("chip-wide loops, median of 5 interleaved runs in this run.  Rows '16x16x32 mix': v_mfma_f32_16x16x32_f16 whose A operands are "
                                             "the LDS reads' data, VALU in the softmax's composition (fma, exp, cvt_pk, pk_max3) at the density named, one interleaved stream per "
                                             "wave.  Rows '16x16x32 ping-pong': the forward's two-group structure with the instruction counts of one tile per phase.  Rows 'MFMA + ...': "
                                             "the round-1 probe (v_mfma_f32_32x32x16, constant operands), kept for comparison across rounds")
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_fwd_ceiling_ablations.json")), key=lambda p: int(re.search(r"r(\d+)_", os.path.basename(p)).group(1)))
    abl = None
    for path in reversed(files):
        try:
            with open(path) as f:
                d = json.load(f)
            if workload in d.get("workloads", {}):
                abl = (os.path.basename(path), d, d["workloads"][workload])
                break
        except (OSError, ValueError, KeyError):
            pass
    if abl:
        name, d, w = abl
        out["same_structure_ablated"] = {"source": f"committed profile {name} (timing-only ablation builds, not measured in this run)", "library_source_digest": d.get("library_source_digest"),
                                         "time_ratio_vs_shipped": w["time_ratio_vs_shipped"],
                                         "tflops_scaled_to_this_run": {k: achieved / v for k, v in w["time_ratio_vs_shipped"].items() if v}}
    rows = clock_rows or {}
    pm = rows.get(own)
    d64 = "d64" in workload
    structure, mix = (rows.get(PROBE_PP_D64 if d64 else PROBE_PP_D128), rows.get(PROBE_MIX_D64 if d64 else PROBE_MIX_D128)) if is16 else (None, None)
    chain = [["nominal dense fp16 MFMA peak (256 CUs x 2.4 GHz x 4096 FLOP/clk)", PEAK_DENSE_FP16_TFLOPS]]
    if pm:
        chain.append(["power cap: this MFMA shape alone, pipes 100 % busy, N(0,1) operands", pm])
    if structure:
        chain.append(["this kernel's structure and instruction counts without its dependencies (two-group ping-pong probe: no LDS-DMA, no mask, no causal diagonal, "
                      "no prologue / epilogue, straight-line softmax)", structure])
    chain.append(["shipped kernel", achieved])
    out["chain_tflops"] = chain
    out["chain_step_ratios"] = [chain[i + 1][1] / chain[i][1] for i in range(len(chain) - 1)]
    out["frac_of_power_capped_mfma_rate"] = achieved / pm if pm else None
    out["shipped_over_structure_probe"] = achieved / structure if structure else None
    if structure:
        # the probe's rate counts every MFMA it issues (68 per wave and step, the 4 row-sum MFMAs of the MFMA-summed tiles included); `achieved` counts algorithmic FLOPs (64 per step)
        out["structure_probe_accounting"] = {
            "probe_mfma_per_wave_step": PROBE_PP_MFMA_ISSUED, "algorithmic_mfma_per_wave_step": PROBE_PP_MFMA_ALGORITHMIC,
            "structure_probe_algorithmic_tflops": structure * PROBE_PP_MFMA_ALGORITHMIC / PROBE_PP_MFMA_ISSUED,
            "shipped_over_structure_probe_same_accounting": achieved / (structure * PROBE_PP_MFMA_ALGORITHMIC / PROBE_PP_MFMA_ISSUED),
            "note": "like for like: the probe's TFLOP/s x 64 / 68 (its row-sum MFMAs are not attention FLOPs; the shipped kernel issues the same 68 on its MFMA-summed fp16 tiles and is "
                    "credited 64).  In cycles the steady loops are closer still: profiles/r6_fwd16_phase_timing.log, ~2750 per step against the probe's 2624",
        }
    out["shipped_over_mixed_stream_probe"] = achieved / mix if mix else None
    out["mixed_stream_probe_tflops"] = mix
    return out


def run_clockbench(argv, timeout=240):
    import subprocess

    exe = os.path.join(ROOT, "tools", "clockbench")
    if not os.path.exists(exe):
        return None
    return subprocess.run([exe] + list(argv), capture_output=True, text=True, timeout=timeout).stdout


def power_capped_mfma_rate(seconds=1.0):
    """the denominator of `frac_of_power_capped_mfma_rate`, at SETTLED power: ONE launch of the chip-wide v_mfma_f32_16x16x32 loop lasting >= `seconds`
    (tools/clockbench --rows ... --seconds: VERDICT r5 item 7 - the 25 ms launches of the full table read the first moments of a load step)"""
    try:
        text = run_clockbench(["--rows", PROBE_PURE16, "--seconds", str(seconds), "--reps", "1"])
        rows = parse_clockbench_rows(text or "")
        return rows.get(PROBE_PURE16)
    except Exception:  # noqa: BLE001 - the line reports None
        return None


def measured_mfma_ceiling():
    """tools/clockbench (built by __graft_entry__.build()): TFLOP/s of a chip-wide back-to-back MFMA loop on random operands
    = what the MFMA roof really is on this box under its power limit (median of 5 interleaved runs).  Reported next to the
    nominal 2.5 PFLOP/s, never used as `peak`."""
    try:
        text = run_clockbench([])
        if text is None:
            return {"error": "tools/clockbench not built"}
        res = parse_clockbench(text)
        res["rows"] = parse_clockbench_rows(text)
        return res
    except Exception as e:  # noqa: BLE001 - reported, not hidden
        return {"error": f"{type(e).__name__}: {e}"}


def cpu_baseline(args):
    """CPU oracle (kind 'port') on a bounded sample of the headline workload + torch SDPA math path."""
    import numpy as np
    import torch
    from oracle import attn_oracle as A

    b, s, h, d = 1, args.cpu_sample_seq, A.num_threads(), 128      # one head per host thread
    rng = np.random.default_rng(0)
    q, k, v = (A.round_lp(rng.standard_normal((b, s, h, d)), A.ROUND_FP16) for _ in range(3))
    t0 = time.perf_counter()
    A.attn_fwd(q, k, v, causal=True, round_mode=A.ROUND_FP16)
    dt = time.perf_counter() - t0
    port = {
        "value": fwd_flops(b, s, s, h, d, True) / dt / 1e12, "unit": "TFLOP/s", "cores": A.num_threads(), "kind": "port",
        "sample": f"oracle/attn_oracle.c forward, b={b} h={h} seq={s} d={d} fp16-rounded causal "
                  f"(same per-head problem as the headline, shortened from seq 16384), {dt:.1f} s",
    }
    # north_star: PyTorch SDPA CPU math path at BASELINE configs[0] (b1 s512 h4 d128 fp32), same run
    from torch.nn.attention import SDPBackend, sdpa_kernel

    qt, kt, vt = (torch.randn(1, 4, 512, 128) for _ in range(3))
    n = 20
    full_threads = torch.get_num_threads()
    with sdpa_kernel(SDPBackend.MATH):
        # configs[0] is a 0.5 GFLOP problem: with every host thread in the pool it measures thread-pool overhead, not arithmetic (the
        # 4x larger s1024 point of the same path ran 3x FASTER on one box).  So the thread count is swept and the baseline is the BEST point; the
        # full-pool figure stays in the record, marked for what it is.
        sweep = {}
        for nt in sorted({1, 4, 16, 64, full_threads}):
            if nt > full_threads:
                continue
            torch.set_num_threads(nt)
            for _ in range(3):
                torch.nn.functional.scaled_dot_product_attention(qt, kt, vt)
            t0 = time.perf_counter()
            for _ in range(n):
                torch.nn.functional.scaled_dot_product_attention(qt, kt, vt)
            sweep[nt] = (time.perf_counter() - t0) / n
        torch.set_num_threads(full_threads)
        best_threads = min(sweep, key=sweep.get)
        dt, dt_full = sweep[best_threads], sweep[full_threads]
        # a bounded ladder towards the GPU shapes (the math path materialises b*h*s*s fp32 scores: 137 GB at the headline shape)
        ladder = {}
        for ss, hh in ((1024, 4), (2048, 4), (2048, 32)):
            ql, kl, vl = (torch.randn(1, hh, ss, 128) for _ in range(3))
            torch.nn.functional.scaled_dot_product_attention(ql, kl, vl)
            t1 = time.perf_counter()
            reps = 3
            for _ in range(reps):
                torch.nn.functional.scaled_dot_product_attention(ql, kl, vl)
            dl = (time.perf_counter() - t1) / reps
            ladder[f"b1_h{hh}_s{ss}"] = {"ms": dl * 1e3, "tflops": fwd_flops(1, ss, ss, hh, 128, False) / dl / 1e12}
    # the baseline the north star names: PyTorch SDPA, CPU, math path, on this node's host cores, in the same run
    f0 = fwd_flops(1, 512, 512, 4, 128, False)
    out = {"value": f0 / dt / 1e12, "unit": "TFLOP/s", "cores": best_threads, "kind": "sdpa_math_cpu",
           "host_cores": os.cpu_count(),
           "sample": f"torch.nn.functional.scaled_dot_product_attention under sdpa_kernel(MATH) on CPU tensors, b1 s512 h4 d128 fp32 non-causal "
                     f"(BASELINE configs[0]), mean of {n} calls = {dt * 1e3:.2f} ms at the best thread count of the sweep ({best_threads} torch threads of {os.cpu_count()} host cores)",
           "thread_sweep_ms": {str(k_): v_ * 1e3 for k_, v_ in sweep.items()},
           "full_pool": {"threads": full_threads, "ms": dt_full * 1e3, "tflops": f0 / dt_full / 1e12,
                         "note": "overhead-bound: a 0.5 GFLOP problem on the whole thread pool times the pool, not the arithmetic"},
           "ladder_same_path": ladder, "oracle_port": port}
    return out


def contract_fields(workload, world):
    """The workload-naming part of the contract line, ONE statement for the measured path and for --fake-step (tests/test_dist_cpu.py launches the
    driver's SCALE command line against it): per-GPU work is fixed as N grows (weak scaling), so the whole job at N = 8 is b = 32."""
    b, s, h, hk, d, dtype, causal, backward = WORKLOADS[workload]
    return {"higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16" if dtype == "fp16" else "bf16", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[{ {'c2': 1, 'c3': 2, 'c4': 3, 'c5shard': 4}[workload] }] per GPU: "
                                   f"{'fwd+bwd' if backward else 'fwd'} b={b} seq={s} h={h} h_k={hk} d={d} {dtype} "
                                   f"{'causal' if causal else 'non-causal'}",
                       "global_batch": b * world, "seq_len": s, "parallelism": f"batch-sharded x{world}, no collective",
                       "flops_def": "4*b*h*sq*sk*d (x0.5 causal) [SURVEY.md 8d]"}}


def headline_fields(args, dist, backward, flops_rank, wall, comm_backend, capi, prop):
    """The result line of every run: the headline rate of the K timed steps and what names it (a --full run adds its measurements to it)"""
    value = flops_rank * dist.world / (wall / args.steps) / 1e12
    return {"metric": "attention_fwd_tflops" if not backward else "attention_fwd_bwd_tflops",
            "value": value, "unit": "TFLOP/s", "n_gpus": dist.world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": wall / args.steps * 1e3, **contract_fields(args.workload, dist.world),
            "frac_of_fp16_mfma_peak": value / (PEAK_DENSE_FP16_TFLOPS * dist.world),
            "comm_backend": comm_backend, "library": capi.lib().fa_build_info().decode(), "git_commit": build_commit(),
            "device": {"name": prop.name or getattr(prop, "gcnArchName", ""), "arch": getattr(prop, "gcnArchName", ""), "cus": prop.multi_processor_count,
                       "hbm_gib": prop.total_memory / 2**30, "peak_used_tflops": PEAK_DENSE_FP16_TFLOPS}}


DUMP_BUDGET_ELEMS = 15 << 20      # --dump-outputs: 60 MiB of float32 over all arrays


def dump_outputs(torch, outdir, tensors):
    """--dump-outputs: every tensor as outdir/<name>.npy in float32.  One larger than its share of DUMP_BUDGET_ELEMS is sampled: a fixed set of rows of its
    last dimension (seeded permutation, sorted), the same in every run with the same arguments, saved as a (rows, last dim) array."""
    import numpy as np

    os.makedirs(outdir, exist_ok=True)
    share = DUMP_BUDGET_ELEMS // len(tensors)
    for name, x in tensors.items():
        if x.numel() > share:
            rows = x.reshape(-1, x.shape[-1])
            pick = torch.randperm(rows.shape[0], generator=torch.Generator().manual_seed(0))[:share // x.shape[-1]].sort().values
            x = rows.index_select(0, pick.to(x.device))
        np.save(os.path.join(outdir, name + ".npy"), x.float().cpu().numpy())


def c5_weak_config(world):
    """BASELINE configs[4] as the N > 1 runs carry it in `extra.c5_weak_noncausal_16k`: b = 4 per rank, i.e. the configuration's b = 32 at N = 8"""
    eb, es, eh, _, ed, edt, ec, _ = WORKLOADS["c5shard"]
    return f"BASELINE configs[4] shape: fwd b={eb * world} (4 per rank) seq={es} h={eh} d={ed} {edt} {'causal' if ec else 'non-causal'}"


def run_fake(args, dist):
    """--fake-step: no GPU, no kernels — exercises sharding, timing aggregation, the strong-scaling sweep bookkeeping and the
    nccl -> gloo fallback under gloo (CPU tests)."""
    from flash_attn_turing.sharding import plan_shards

    backend = dist.comm_backend
    if dist.enabled and dist.want == "nccl":
        try:
            import torch

            backend = dist.try_nccl(torch.device("cuda", 0))      # no GPU on the CPU box: must come back as gloo + reason
        except Exception as e:  # noqa: BLE001
            backend = f"gloo (nccl probe raised {type(e).__name__})"
    plan = plan_shards(4 * dist.world, 32, 32, dist.world)[dist.rank]
    step = lambda: time.sleep(0.002 * (1 + dist.rank))
    wall, local = timed_region(step, args.steps, args.warmup, dist, lambda: None)
    units = dist.reduce_sum(float(plan.n_units))

    def make_point(seq, causal, p):
        # a fake kernel whose time is proportional to the (batch, head) units of the shard it is given
        per_unit = 8e-5 * (seq / 512.0)      # (5-10 ms per fake launch: long against the sleep jitter of a busy CI box)
        return (lambda: time.sleep(per_unit * p.n_units)), (lambda: time.sleep(per_unit * 4 * 32))

    sweep = strong_scaling_sweep(dist, make_point, lambda: None, None, seqs=(512, 1024), causals=(False,))
    if dist.rank == 0:
        extra = {"sweep_strong": sweep}
        if dist.world > 1:
            extra["c5_weak_noncausal_16k"] = {"config": c5_weak_config(dist.world)}
        line = {"metric": "fake_units_per_s", "value": units * args.steps / wall, "unit": "units/s",
                "n_gpus": dist.world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": wall / args.steps * 1e3, "units_total": units, "local_ms": local * 1e3,
                "comm_backend": backend, "subgroup_collectives": dist.sub_calls, "extra": extra}
        line.update(contract_fields(args.workload, dist.world))
        line["data"] = "none (--fake-step: harness self-test, no kernels)"
        print(json.dumps(line))


def bwd_rooflines(torch, capi, et, causal, b, s, h, d):
    """Per-kernel roofline entries of the backward (C4): dot_do_o is HBM-bound, dQ and dK/dV are MFMA-bound; each timed alone with
    HIP events through its stage-level C-ABI entry point.  `executed` FLOPs include the S / dP recomputation (6 and 8 x sq*sk*d
    per head); the algorithmic backward FLOPs (2.5 x forward) are what `bwd_tflops` uses."""
    p = capi.bwd_params(et["q"], et["k"], et["v"], et["o"], et["lse"], et["dout"], et["dq"], et["dk"], et["dv"], et["dsum"], causal)
    dtype_name = "bf16" if et["q"].dtype == torch.bfloat16 else "fp16"
    ws = capi.attach_workspace(p, et["q"])      # noqa: F841  (dK/dV scratch for GQA / MQA shapes; None at the MHA bench shapes)
    pair = b * h * float(s) * s * (0.5 if causal else 1.0)
    out = {}
    for name, kern, flop_mult in (("dot_do_o", "fa_bwd_dot_do_o_kernel", 0), ("dq", capi.kernel_name("dq", b, s, s, h, d, causal, dtype_name), 6),
                                  ("dkdv", capi.kernel_name("dkdv", b, s, s, h, d, causal, dtype_name), 8)):
        f = lambda: capi.bwd_stage(name, p)
        f(); torch.cuda.synchronize()
        ms = event_time_ms(torch, f, 5, reps=5)
        if flop_mult == 0:
            byts = 2.0 * b * s * h * d * 2 + b * h * s * 4.0           # read O and dO once, write D
            gbps = byts / ms / 1e6
            out[name] = {"kernel": kern, "bound": "hbm", "avg_launch_ms": ms, "achieved": gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                         "frac": gbps / PEAK_HBM_GBPS, "algorithmic_bytes_per_launch": byts,
                         "note": "stand-alone entry point; fa_run_mha_bwd (what bwd_ms times) computes D inside the dQ kernel and does not launch it"}
        else:
            tf = flop_mult * pair * d / ms / 1e9
            out[name] = {"kernel": kern, "bound": "mfma", "avg_launch_ms": ms, "achieved": tf, "peak": PEAK_DENSE_FP16_TFLOPS,
                         "unit": "TFLOP/s", "frac": tf / PEAK_DENSE_FP16_TFLOPS, "executed_flops_per_launch": flop_mult * pair * d}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults (round 4): 300 warm-up steps = ~2 s of the headline launch, so that the 100 timed steps run at the clock and package power the
    # chip SETTLES at (round 3's 5 + 20 were timed while the power was still ramping: 917 W mean against 1.33 kW sustained, 2 % optimistic)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--fake-step", action="store_true", help="CPU-only harness self-test (no kernels)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: roofline, cpu_baseline, the other BASELINE configs, sweeps, ceiling probes (without it: warm-up, "
                         "the timed steps and the result line only)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the arrays the last timed step computed (rank 0) as DIR/<name>.npy, float32; arrays too large for the 60 MiB budget "
                         "as a fixed, seeded sample of their rows")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the other BASELINE configs")
    ap.add_argument("--n1-consistency", action="store_true", help="with --full --no-extra: still run the N = 1 row of the strong-scaling sweep beside the headline (extra.n1_consistency)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-sample-seq", type=int, default=4096)
    args = ap.parse_args()
    if args.n1_consistency and not args.full:
        ap.error("--n1-consistency is a measurement of --full")
    if args.dump_outputs and args.fake_step:
        ap.error("--dump-outputs needs the kernels: --fake-step computes nothing")

    dist = Dist(args.backend)
    if dist.world != args.gpus and dist.world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={dist.world}")
    if args.gpus > 1 and dist.world == 1:
        raise SystemExit("for --gpus N>1 launch one rank per GPU with torch.distributed.run (see module docstring)")
    if args.fake_step:
        run_fake(args, dist)
        dist.close()
        return

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU: the hot path is HIP-only, there is no CPU fallback")
    from flash_attn_turing import capi   # fails loudly if the HIP build is missing
    from flash_attn_turing.sharding import shard_tensor

    # one rank per GPU; the modulo only matters when the harness itself is exercised with more ranks
    # than devices (e.g. --backend gloo with 2 ranks on a 1-GPU box)
    # --gpus N means N GPUs: say so before anything is allocated (FA_BENCH_ALLOW_OVERSUBSCRIBE=1 keeps the harness exercise of
    # several ranks on one device, e.g. `--backend gloo` with 2 ranks on a 1-GPU box)
    n_dev = torch.cuda.device_count()
    if n_dev < args.gpus and os.environ.get("FA_BENCH_ALLOW_OVERSUBSCRIBE") != "1":
        raise SystemExit(f"bench.py --gpus {args.gpus}: only {n_dev} ROCm device(s) visible on this node "
                         f"(rank {dist.rank}, LOCAL_RANK {dist.local_rank}); one rank per GPU is required")
    device = torch.device("cuda", dist.local_rank % n_dev)
    torch.cuda.set_device(device)
    comm_backend = dist.try_nccl(device)
    b, s, h, hk, d, dtype, causal, backward = WORKLOADS[args.workload]
    t = make_inputs(torch, device, b, s, h, hk, d, dtype, 1234 + dist.rank, backward)

    def step():
        capi.mha_fwd(t["q"], t["k"], t["v"], t["o"], t["lse"], causal)
        if backward:
            capi.mha_bwd(t["q"], t["k"], t["v"], t["o"], t["lse"], t["dout"], t["dq"], t["dk"], t["dv"], t["dsum"], causal)

    sync = lambda: torch.cuda.synchronize(device)
    flops_rank = fwd_flops(b, s, s, h, d, causal) * (3.5 if backward else 1.0)
    outputs = {n: t[n] for n in (("o", "lse", "dq", "dk", "dv") if backward else ("o", "lse"))}      # what a caller of the step receives
    prop = torch.cuda.get_device_properties(device)
    if not args.full:
        wall, _ = timed_region(step, args.steps, args.warmup, dist, sync, device)
        if args.dump_outputs and dist.rank == 0:
            dump_outputs(torch, args.dump_outputs, outputs)
        if dist.rank == 0:
            print(json.dumps(headline_fields(args, dist, backward, flops_rank, wall, comm_backend, capi, prop)))
        dist.close()
        return
    # the power-capped MFMA rate of this box, >= 1 s at settled power, BEFORE the timed region (and again after it, below): the box-independent denominator
    pm_before = power_capped_mfma_rate() if (dist.rank == 0 and dist.world == 1 and not args.no_extra) else None
    region_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    with PowerSampler(device.index) as sampler:
        wall, _ = timed_region(step, args.steps, args.warmup, dist, sync, device, events=region_events)
        t_reg1 = time.perf_counter()
        if args.dump_outputs and dist.rank == 0:
            dump_outputs(torch, args.dump_outputs, outputs)      # (before the sustained launches below run the step again)
        power_timed = sampler.summary(t_reg1 - wall, t_reg1, f"the timed region itself ({args.steps} steps, {wall * 1e3:.0f} ms)")
        # the timed region of the default command is ~0.15 s; >= 2 s of the same step, every step between its own HIP events, gives the
        # sensors time to settle and the steady-state figure (median / min) SURVEY 8(d) asks for
        t_s0 = time.perf_counter()
        sustained_evs = []
        while time.perf_counter() - t_s0 < 2.0:
            for _ in range(10):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                sustained_evs.append((e0, e1))
            sync()
        t_s1 = time.perf_counter()
        power_sustained = sampler.summary(t_s0 + 0.5, t_s1, "2 s of back-to-back launches of the same step right after the timed region (first 0.5 s dropped)")
    ms_per_step = wall / args.steps * 1e3
    region_event_ms = region_events[0].elapsed_time(region_events[1]) / args.steps      # device-side ms per step of the timed region
    import statistics as _stats
    sus = [a.elapsed_time(b) for a, b in sustained_evs][len(sustained_evs) // 4:]      # (first quarter dropped: the ramp)
    sustained = {"what": "every step of >= 2 s of back-to-back steps right after the timed region, each between its own HIP events (first quarter dropped)",
                 "steps": len(sus), "seconds": t_s1 - t_s0, "median_ms": _stats.median(sus), "min_ms": min(sus), "max_ms": max(sus),
                 "tflops_at_median": flops_rank / _stats.median(sus) / 1e9, "tflops_at_min": flops_rank / min(sus) / 1e9,
                 "frac_at_median": flops_rank / _stats.median(sus) / 1e9 / PEAK_DENSE_FP16_TFLOPS}

    # dominant-kernel roofline: the forward kernel.  ONE definition: `achieved` = algorithmic FLOPs of a launch over the
    # kernel's average launch duration, HIP events on the launch stream OVER THE TIMED REGION - for a forward-only workload a step IS one
    # launch of that kernel, so achieved follows from the same K launches as `value` / `ms_per_step` (they differ by the host-side bracket
    # only: barrier + synchronize).  A forward+backward workload times its forward launches alone in a loop of the same length.
    fwd_kernel = capi.kernel_name("fwd", b, s, s, h, d, causal, dtype)      # the kernel THIS workload's launches go to (the choice can depend on the dtype: ADVICE r4)
    fwd_only = lambda: capi.mha_fwd(t["q"], t["k"], t["v"], t["o"], t["lse"], causal)
    k_ms = region_event_ms if not backward else event_time_ms(torch, fwd_only, max(5, args.steps))
    k_tflops = fwd_flops(b, s, s, h, d, causal) / (k_ms * 1e-3) / 1e12
    k_dist = launch_time_distribution(torch, fwd_only, max(30, args.steps))
    traffic, traffic_source, prof_digest, prof_commit = hbm_traffic_from_profile(args.workload, fwd_kernel) if dist.rank == 0 else (None, None, None, None)
    lib_digest = library_source_digest(capi)
    sclk_ghz = max(capi.device_clock_khz(device.index), 0) / 1e6     # hipDeviceAttributeClockRate (torch's props carry no clock)
    roofline = {"bound": "mfma", "kernel": fwd_kernel, "achieved": k_tflops, "peak": PEAK_DENSE_FP16_TFLOPS,
                "unit": "TFLOP/s", "frac": k_tflops / PEAK_DENSE_FP16_TFLOPS,
                "traffic": traffic, "traffic_source": traffic_source,
                "traffic_profile_library_digest": prof_digest, "traffic_profile_git_commit": prof_commit, "library_source_digest": lib_digest,
                "profile_matches_library": (prof_digest == lib_digest) if prof_digest else None,
                "avg_launch_ms": k_ms, "avg_launch_ms_source": ("HIP events around the K steps of the timed region" if not backward else "separate loop of forward launches (the step holds backward kernels too)"),
                "frac_from_ms_per_step": fwd_flops(b, s, s, h, d, causal) / (ms_per_step * 1e-3) / 1e12 / PEAK_DENSE_FP16_TFLOPS if not backward else None,
                "sustained": sustained, "launch_ms_distribution": k_dist,
                "tflops_at_median_launch": fwd_flops(b, s, s, h, d, causal) / k_dist["median_ms"] / 1e9,
                "tflops_at_min_launch": fwd_flops(b, s, s, h, d, causal) / k_dist["min_ms"] / 1e9,
                "power_and_sclk": {"timed_region": power_timed, "sustained": power_sustained},
                "algorithmic_flops_per_launch": fwd_flops(b, s, s, h, d, causal),
                "algorithmic_hbm_gbps": fwd_bytes(b, s, s, h, hk, d) / (k_ms * 1e-3) / 1e9,
                "peak_derivation": {"cus": prop.multi_processor_count, "sclk_ghz": sclk_ghz, "flop_per_clk_per_cu": MFMA_FLOP_PER_CLK_PER_CU,
                                    "cus_x_sclk_x_4096_tflops": prop.multi_processor_count * sclk_ghz * MFMA_FLOP_PER_CLK_PER_CU / 1e3}}

    extra = {}
    state = {}

    def make_point(seq, cz, plan):
        # whole tensors on every rank (same seed), the rank's shard = strided views of them (no copy)
        if state.get("seq") != seq:
            state.clear()
            torch.cuda.empty_cache()
            w = make_inputs(torch, device, 4, seq, 32, 32, 128, "fp16", 99, False)
            qs, os_ = shard_tensor(w["q"], plan, False), shard_tensor(w["o"], plan, False)
            ks, vs = shard_tensor(w["k"], plan, True), shard_tensor(w["v"], plan, True)
            lse_s = torch.empty(qs.shape[0], qs.shape[2], seq, device=device, dtype=torch.float32)
            state.update(seq=seq, w=w, shard=(qs, ks, vs, os_, lse_s))
        w, (qs, ks, vs, os_, lse_s) = state["w"], state["shard"]
        ps = capi.fwd_params(qs, ks, vs, os_, lse_s, cz) if qs.numel() else None
        pw = capi.fwd_params(w["q"], w["k"], w["v"], w["o"], w["lse"], cz)
        return (lambda: capi.run_fwd(ps) if ps is not None else None), (lambda: capi.run_fwd(pw))

    if args.workload == "c3" and dist.world == 1 and (args.n1_consistency or not args.no_extra):
        # N = 1 consistency: the driver derives scaling efficiency from the headline `value` of its N = 1, 2, 4, 8 runs, the line's own strong-scaling
        # sweep from its in-run single-GPU reference.  At N = 1 the shard IS the whole problem and the sweep's 16k-causal point is the headline workload through the OTHER code
        # path (plan_shards -> shard views -> run_fwd on prepared params under the whole problem's policy): the two must tell the same rate, or the first real SCALE run would
        # debut a harness discrepancy together with RCCL.  Two consecutive 0.14 s windows on this chip differ by up to 4 % whatever they run (the clock follows the package
        # power, which follows the last second's history), so the three step functions are timed INTERLEAVED, 4 rounds x 40 launches each between the same barrier + sync
        # brackets, and compared by their medians.  tests/test_perf_relations_gpu.py asserts 1 %.
        from flash_attn_turing.sharding import plan_shards, problem_policy
        import statistics as _st

        step_shard_own, step_whole = make_point(s, causal, plan_shards(4, 32, 32, 1)[0])

        def step_shard():
            with problem_policy(4, 32):
                step_shard_own()

        arms = {"headline_step": step, "sweep_shard_path": step_shard, "sweep_whole_path": step_whole}
        times = {k: [] for k in arms}
        for _ in range(4):
            for name, fn in arms.items():
                w_, _ = timed_region(fn, 40, 3, dist, sync, device)
                times[name].append(w_ / 40 * 1e3)
        med = {k: _st.median(v) for k, v in times.items()}
        fl = fwd_flops(b, s, s, h, d, causal)
        state.clear()
        torch.cuda.empty_cache()
        extra["n1_consistency"] = {"what": "the headline step, the strong-scaling sweep's shard path at N = 1 and its whole-problem path: 4 interleaved rounds x 40 launches each, medians",
                                   "median_ms": med, "tflops": {k: fl / v / 1e9 for k, v in med.items()}, "ms_per_round": times,
                                   "shard_path_over_headline": med["headline_step"] / med["sweep_shard_path"],
                                   "whole_path_over_headline": med["headline_step"] / med["sweep_whole_path"]}
    if not args.no_extra and dist.world > 1:
        del t
        torch.cuda.empty_cache()

        extra["sweep_strong_b4_h32_d128_fp16"] = strong_scaling_sweep(dist, make_point, sync, device)
        state.clear()
        torch.cuda.empty_cache()
        # BASELINE configs[4]: forward, b=32 (= 4 per rank at N=8), seq 16384, non-causal, weak-scaled over the ranks
        eb, es, eh, ehk, ed, edt, ec, _ = WORKLOADS["c5shard"]
        et = make_inputs(torch, device, eb, es, eh, ehk, ed, edt, 777 + dist.rank, False)
        f = lambda: capi.mha_fwd(et["q"], et["k"], et["v"], et["o"], et["lse"], ec)
        w5, _ = timed_region(f, 6, 2, dist, sync, device)
        if dist.rank == 0:
            agg = fwd_flops(eb, es, es, eh, ed, ec) * dist.world * 6 / w5 / 1e12
            extra["c5_weak_noncausal_16k"] = {"config": c5_weak_config(dist.world),
                                              "ms": w5 / 6 * 1e3, "aggregate_tflops": agg, "frac_of_fp16_mfma_peak": agg / (PEAK_DENSE_FP16_TFLOPS * dist.world)}
        del et
    if not args.no_extra and dist.rank == 0 and dist.world == 1:
        del t
        torch.cuda.empty_cache()
        for name, (eb, es, eh, ehk, ed, edt, ec, ebwd) in WORKLOADS.items():
            if name == args.workload:
                continue
            et = make_inputs(torch, device, eb, es, eh, ehk, ed, edt, 4321, ebwd)
            f = lambda: capi.mha_fwd(et["q"], et["k"], et["v"], et["o"], et["lse"], ec)
            f(); sync()
            ms = event_time_ms(torch, f, 5, reps=5)
            ff = fwd_flops(eb, es, es, eh, ed, ec)
            extra[name] = {"fwd_ms": ms, "fwd_tflops": ff / ms / 1e9, "fwd_frac_peak": ff / ms / 1e9 / PEAK_DENSE_FP16_TFLOPS}
            if ebwd:
                g = lambda: capi.mha_bwd(et["q"], et["k"], et["v"], et["o"], et["lse"], et["dout"], et["dq"], et["dk"],
                                         et["dv"], et["dsum"], ec)
                g(); sync()
                bms = event_time_ms(torch, g, 3, reps=5)
                extra[name].update({"bwd_ms": bms, "bwd_tflops": 2.5 * ff / bms / 1e9,
                                    "fwd_bwd_tflops": 3.5 * ff / (ms + bms) / 1e9,
                                    "roofline_bwd": bwd_rooflines(torch, capi, et, ec, eb, es, eh, ed)})
            del et
            torch.cuda.empty_cache()
        # GQA / MQA backward under a causal mask (b4 s8192 h32 d128 bf16): few KV heads shrink and unbalance the dK/dV grid; with the
        # ABI-3 workspace the launch splits a KV head's query-head group over workgroups.  Same FLOPs in every row.
        gq = {}
        for hk_ in (32, 8, 1):
            et = make_inputs(torch, device, 4, 8192, 32, hk_, 128, "bf16", 555, True)
            capi.mha_fwd(et["q"], et["k"], et["v"], et["o"], et["lse"], True)
            pb = capi.bwd_params(et["q"], et["k"], et["v"], et["o"], et["lse"], et["dout"], et["dq"], et["dk"], et["dv"], et["dsum"], True)
            g = lambda: capi.run_bwd(pb)
            g(); sync()
            single = event_time_ms(torch, g, 3, reps=3)
            ws = capi.attach_workspace(pb, et["q"])
            g(); sync()
            split = event_time_ms(torch, g, 3, reps=3) if ws is not None else single
            gq[f"h32_hk{hk_}"] = {"bwd_ms": split, "bwd_ms_without_workspace": single, "workspace_bytes": 0 if ws is None else ws.numel() * 4,
                                  "bwd_tflops": 2.5 * fwd_flops(4, 8192, 8192, 32, 128, True) / split / 1e9}
            del et, pb, ws
            torch.cuda.empty_cache()
        for v_ in gq.values():
            v_["vs_mha"] = v_["bwd_ms"] / gq["h32_hk32"]["bwd_ms"]
        extra["gqa_bwd_b4_s8192_d128_bf16_causal"] = gq
        # head_dim 64, the reference's other instantiation (flash_*_hdim64_*): b4 s8192 h32 fp16, forward and backward
        d64 = {}
        for cz in (False, True):
            et = make_inputs(torch, device, 4, 8192, 32, 32, 64, "fp16", 4321, True)
            f = lambda: capi.mha_fwd(et["q"], et["k"], et["v"], et["o"], et["lse"], cz)
            g = lambda: capi.mha_bwd(et["q"], et["k"], et["v"], et["o"], et["lse"], et["dout"], et["dq"], et["dk"], et["dv"], et["dsum"], cz)
            f(); g(); sync()
            fms, bms = event_time_ms(torch, f, 5, reps=5), event_time_ms(torch, g, 3, reps=5)
            ff = fwd_flops(4, 8192, 8192, 32, 64, cz)
            d64["causal" if cz else "noncausal"] = {"fwd_ms": fms, "fwd_tflops": ff / fms / 1e9, "bwd_ms": bms, "bwd_tflops": 2.5 * ff / bms / 1e9}
            del et
            torch.cuda.empty_cache()
        extra["d64_b4_s8192_h32_fp16"] = d64
        # head_dim 128 has two kernel sets (32x32x16 / 16x16x32 MFMA tiles; fa_set_kernel_policy): the two pinned, interleaved in this process, on
        # the headline forward and on the configs[3] backward - what the default policy's choice is worth ON THIS BOX (it moves by a few %
        # between boxes of the pool); the policy is back on FA_POLICY_AUTO afterwards
        import statistics as _st
        ab = {}
        for label, (bb, ss, hh, dt_, cz, bw) in {"c3_fwd": (4, 16384, 32, "fp16", True, False), "c4_bwd": (4, 8192, 32, "bf16", False, True)}.items():
            et = make_inputs(torch, device, bb, ss, hh, hh, 128, dt_, 777, bw)
            capi.mha_fwd(et["q"], et["k"], et["v"], et["o"], et["lse"], cz)
            f = ((lambda: capi.mha_bwd(et["q"], et["k"], et["v"], et["o"], et["lse"], et["dout"], et["dq"], et["dk"], et["dv"], et["dsum"], cz)) if bw
                 else (lambda: capi.mha_fwd(et["q"], et["k"], et["v"], et["o"], et["lse"], cz)))
            times = {capi.POLICY_MFMA32: [], capi.POLICY_MFMA16: [], capi.POLICY_AUTO: []}
            try:
                for _ in range(5):
                    for pol in times:
                        capi.set_kernel_policy(pol)
                        f(); sync()
                        times[pol].append(event_time_ms(torch, f, 3))
            finally:
                capi.set_kernel_policy(capi.POLICY_AUTO)
            m32, m16, mauto = (_st.median(times[pol]) for pol in (capi.POLICY_MFMA32, capi.POLICY_MFMA16, capi.POLICY_AUTO))
            stages = ("dq", "dkdv") if bw else ("fwd",)
            picks = {st_: capi.kernel_name(st_, bb, ss, ss, hh, 128, cz, dt_) for st_ in stages}
            ab[label] = {"ms_mfma_32x32x16": m32, "ms_mfma_16x16x32": m16, "ms_auto": mauto, "ratio_16_over_32": m16 / m32,
                         "ratio_auto_over_best_pinned": mauto / min(m32, m16), "auto_picks": picks}
            # when AUTO launches exactly the kernels of one pinned set, the two arms time the SAME code: their ratio is this measurement's noise floor
            same = "mfma16" if all("16_kernel" in k_ for k_ in picks.values()) else "mfma32" if not any("16_kernel" in k_ for k_ in picks.values()) else None
            if same is not None:
                ab[label].update({"auto_launches_the_kernels_of": same, "noise_floor_same_kernels_ratio": mauto / (m16 if same == "mfma16" else m32)})
            del et
            torch.cuda.empty_cache()
        extra["kernel_sets_ab"] = ab
        # seqlen sweep of the reference's published chart (README.md:7-16): b4 h32 d128
        for cz in (False, True):
            sweep = {}
            for ss in SWEEP_SEQS:
                et = make_inputs(torch, device, 4, ss, 32, 32, 128, "fp16", 99, False)
                f = lambda: capi.mha_fwd(et["q"], et["k"], et["v"], et["o"], et["lse"], cz)
                f(); sync()
                # windows of >= ~15 ms each (a 20-call window of a 70 us launch right after an idle sync read 0.085 ms on one box, 0.070 on
                # every other measurement of the same kernel: the clock had not come back up); the SDPA comparison gets the same windows
                n_it = max(8, min(400, int(15.0 / max(event_time_ms(torch, f, 10), 1e-3))))
                ms = event_time_ms(torch, f, n_it, reps=3)
                sweep[str(ss)] = {"ms": ms, "tflops": fwd_flops(4, ss, ss, 32, 128, cz) / ms / 1e9, "calls_per_window": n_it}
                # the reference's headline comparison (README.md:16 "around 2x faster than PyTorch attention"), on THIS GPU:
                # PyTorch-ROCm's own fused SDPA on the same tensors ((b,h,s,d) strided views, no copy)
                try:
                    qt, kt, vt = (et[n].permute(0, 2, 1, 3) for n in ("q", "k", "v"))
                    g = lambda: torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, is_causal=cz)
                    g(); sync()
                    sms = event_time_ms(torch, g, max(8, n_it // 2), reps=3)
                    sweep[str(ss)].update({"torch_sdpa_ms": sms, "speedup_vs_torch_sdpa": sms / ms})
                except Exception as exc:  # noqa: BLE001
                    sweep[str(ss)]["torch_sdpa_error"] = str(exc)[:80]
                del et
            extra["sweep_b4_h32_d128_fp16_" + ("causal" if cz else "noncausal")] = sweep

    cpu = None
    if dist.rank == 0 and dist.world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args)

    ceiling = measured_mfma_ceiling() if (dist.rank == 0 and dist.world == 1 and not args.no_extra) else None
    if ceiling is not None:
        roofline["sustained_mfma_peak_measured"] = ceiling          # carries {"error": ...} instead of vanishing if clockbench fails
        if "tflops" in ceiling:
            roofline["frac_of_sustained_measured"] = k_tflops / ceiling["tflops"]          # against the 32x32x16 loop (comparable across rounds)
            if "mfma_16x16x32" in ceiling and "pp16" in fwd_kernel:
                roofline["frac_of_sustained_measured_own_mfma_shape"] = k_tflops / ceiling["mfma_16x16x32"]["tflops"]
    if dist.rank == 0 and dist.world == 1:
        cb = ceiling_block(args.workload, fwd_kernel, k_tflops, (ceiling or {}).get("rows"))
        roofline["ceiling"] = cb
        # box-independent figures at the TOP level of `roofline` (scalars: the driver's parsed record keeps them), VERDICT r5 item 7
        pm_after = power_capped_mfma_rate() if not args.no_extra else None
        pms = [x for x in (pm_before, pm_after) if x]
        if "pp16" in fwd_kernel and pms:
            pm_mean = sum(pms) / len(pms)
            roofline["power_capped_mfma_rate_tflops_before"] = pm_before
            roofline["power_capped_mfma_rate_tflops_after"] = pm_after
            roofline["frac_of_power_capped_mfma_rate"] = k_tflops / pm_mean
            roofline["frac_of_power_capped_mfma_rate_at_median_launch"] = roofline["tflops_at_median_launch"] / pm_mean
            roofline["power_capped_mfma_rate_what"] = ("chip-wide loop of v_mfma_f32_16x16x32_f16 on N(0,1) operands, one launch of >= 1 s at settled power before and one after "
                                                       "the timed region (tools/clockbench --seconds 1); the frac uses their mean")
        roofline["structure_probe_tflops"] = cb["chain_tflops"][2][1] if len(cb["chain_tflops"]) == 4 else None
        roofline["shipped_over_structure_probe"] = cb.get("shipped_over_structure_probe")
        roofline["shipped_over_structure_probe_same_accounting"] = (cb.get("structure_probe_accounting") or {}).get("shipped_over_structure_probe_same_accounting")
        roofline["mixed_stream_probe_tflops"] = cb.get("mixed_stream_probe_tflops")
        roofline["shipped_over_mixed_stream_probe"] = cb.get("shipped_over_mixed_stream_probe")
        if extra.get("d64_b4_s8192_h32_fp16") is not None and ceiling and ceiling.get("rows"):
            # head_dim 64: twice the VALU work per FLOP - its own probes
            rws = ceiling["rows"]
            d64e = extra["d64_b4_s8192_h32_fp16"]
            d64e["ceiling_probes_tflops"] = {"structure (two-group ping-pong, 190 VALU per phase)": rws.get(PROBE_PP_D64), "mixed stream (5.2 VALU + 1 KiB LDS per 32768 FLOP)": rws.get(PROBE_MIX_D64),
                                             "pure v_mfma_f32_16x16x32": rws.get(PROBE_PURE16)}
            for key in ("noncausal", "causal"):
                if isinstance(d64e.get(key), dict) and rws.get(PROBE_PP_D64):
                    d64e[key]["fwd_over_structure_probe"] = d64e[key]["fwd_tflops"] / rws[PROBE_PP_D64]
                    d64e[key]["fwd_over_structure_probe_same_accounting"] = d64e[key]["fwd_tflops"] / (rws[PROBE_PP_D64] * PROBE_PP_MFMA_ALGORITHMIC / PROBE_PP_MFMA_ISSUED)
    if dist.rank == 0 and prof_digest and prof_digest != lib_digest:
        roofline["warning"] = (f"roofline.traffic comes from a profile of library build src={prof_digest}, this run timed src={lib_digest}: "
                               "re-run tools/round_evidence.sh on the current kernels")
    if dist.rank == 0:
        out = headline_fields(args, dist, backward, flops_rank, wall, comm_backend, capi, prop)
        out.update({
            "tflops_at_median_launch": roofline["tflops_at_median_launch"] * dist.world,      # whole-job rate at the MEDIAN launch of a separate 30+ launch loop (less box noise than the K-step mean)
            "roofline": roofline, "cpu_baseline": cpu, "extra": extra,
        })
        print(json.dumps(out))
    dist.close()


if __name__ == "__main__":
    main()
