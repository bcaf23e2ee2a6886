#!/usr/bin/env python3
"""Headline benchmark: training images/s of the camera-aware depth step at 640x480, bs32 per GPU.

Workload = BASELINE.json configs[1]: baseline_unet (f=64, 31,037,633 params), 1 MI355X, bs32,
480x640, fp32, scale-invariant loss only (CombinedDepthLoss weights 1,0,0,0 — the reference still
evaluates all four terms, and so do we).  One step = TensorBoardTrainerEnhanced::trainEpoch's body
(enhanced.h:287-304): forward, loss + dL/dpred, backward, clip_grad_norm_(1.0), Adam — all in
libcad_hip.so.  Synthetic SUN-RGB-D-shaped batches resident in HBM (data loading excluded).

  python bench.py [--gpus N --steps K --warmup W]      # configs[1] (the headline line), nothing else
  python bench.py --full [...]                          # + roofline, cpu_baseline, parity, other workloads
  python bench.py --dump-outputs DIR [...]              # + the last timed step's outputs as DIR/<name>.npy
  python bench.py --config 3                            # ray+FiLM model, bf16 GEMMs, full loss
  python bench.py --config 4                            # baseline_unet, bf16 GEMMs, full loss
  N>1: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N  (one rank per GPU,
  weak scaling: bs32 per GPU; the gradient exchange is libcad's RCCL communicator — decoder-first
  buckets all-reduced on its own stream while the backward runs, the build/train path; torch.distributed
  only hands over the unique id and keeps the host-side barrier / max-over-ranks clock).

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints the headline
fields (value, ms_per_step, last_loss, config; with N>1 the exchange accounting of the timed steps);
everything below runs only with --full (and is null in a plain run's line).
--dump-outputs DIR: after the timed steps, what the last of them handed its caller (dump_outputs).
roofline: the dominant MFMA kernel (largest total time in the timed
region, timed live with HIP events on its launch stream) against its engine's MFMA ceiling.
cpu_baseline: the oracle restatement (LibTorch CPU, the reference's ATen kernels) on a bounded
sample of the workload on this host's physical cores (plus a thread-count sweep); parity: 10
identical steps on the GPU and the CPU path, compared after step 1 and step 10 (prediction, loss,
eval-mode prediction and abs_rel).  bf16_workloads: bounded runs of the other BASELINE
workloads (configs[2], configs[3]'s and configs[4]'s per-GPU steps) in the same process.
"""
import argparse
import ctypes as C
import gc
import json
import re
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "images/sec (640×480 bs32) at 1/2/4/8 MI355X; abs_rel vs CPU ref"
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 = fp32 vector peak
# S3 engine (gemm_s3.hpp): each fp32 multiply-add costs 6 bf16 products on v_mfma_f32_32x32x16_bf16
# (1024 FLOP/clk/SIMD x 1024 SIMDs x 2.4 GHz = 2516.6 TFLOP/s dense bf16), so its fp32-equivalent
# ceiling is 2516.6 / 6.
BF16_MFMA_PEAK_TFLOPS = 2516.6
# block-scaled MXFP8 (v_mfma_scale_f32_32x32x64_f8f6f4 with E4M3 operands): 2x the bf16 rate
MX8_MFMA_PEAK_TFLOPS = 2 * BF16_MFMA_PEAK_TFLOPS
S3_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / 6.0
HBM_PEAK_GBS = 8000.0
FLOP_PER_IMAGE_480x640_F64 = 1.353646e12   # fwd + dgrad + wgrad (= flop_per_image(64))
WORKLOADS = {2: "baseline_unet train step, configs[1]: bs32/GPU 480x640 fp32 SI-only loss",
             3: "ray+FiLM conditioned U-Net train step, configs[2]: bs32/GPU 480x640 bf16 GEMMs, full loss",
             4: "baseline_unet train step, configs[3] per-GPU step: bs32/GPU 480x640 bf16 GEMMs, full loss "
                "(this 1-GPU leg runs no all-reduce; the DP exchange is timed by --gpus N)"}
PRESETS = {2: ("baseline", "fp32"), 3: ("rayfilm", "bf16"), 4: ("baseline", "bf16")}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--weights", default=None, help="si,grad,smooth,reproj (configs[1]: SI only 1,0,0,0)")
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4),
                    help="BASELINE.json configs[i-1]: 2 = baseline_unet fp32 SI-only (default); 3 = ray+FiLM "
                         "conditioned U-Net, bf16, full loss; 4 = baseline_unet bf16 full loss (DP over --gpus)")
    ap.add_argument("--model", default=None, choices=("baseline", "film", "rayfilm"))
    ap.add_argument("--dtype", default=None, choices=("fp32", "bf16"),
                    help="GEMM arithmetic: fp32 (S3 engine, fp32-accurate) or bf16 operands / fp32 accumulation")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the roofline of the dominant kernel "
                         "(a census step + events in the timed region), the CPU baseline and parity steps, the other "
                         "workloads and the data path (N>1: the DP workloads)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs (prediction, loss terms, gradient norm, a sample of the "
                         "updated parameters) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and parity legs")
    ap.add_argument("--no-extra", action="store_true",
                    help="with --full: skip the bf16 workload legs and the data path")
    ap.add_argument("--exchange", default="rccl", choices=("rccl", "torch"),
                    help="N>1 gradient exchange: libcad's RCCL communicator (the build/train path) or torch.distributed")
    # 1 warm-up + >= 3 timed steps at bs32 480x640, on the job's CPU share
    ap.add_argument("--cpu-sample-batch", type=int, default=32)
    ap.add_argument("--cpu-sample-steps", type=int, default=3)
    a = ap.parse_args()
    preset = {2: ("baseline", "fp32", "1,0,0,0"), 3: ("rayfilm", "bf16", "1,0.1,0.001,0.01"),
              4: ("baseline", "bf16", "1,0.1,0.001,0.01")}[a.config]
    a.model = a.model or preset[0]
    a.dtype = a.dtype or preset[1]
    a.weights = a.weights or preset[2]
    return a


def host_cpu():
    """CPU model, physical core / logical CPU counts of this host, and the CPUs this process may use."""
    model, pairs, logical, phys_id = None, set(), 0, "0"
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                k, _, v = line.partition(":")
                k, v = k.strip(), v.strip()
                if k == "processor":
                    logical += 1
                elif k == "model name" and model is None:
                    model = v
                elif k == "physical id":
                    phys_id = v
                elif k == "core id":
                    pairs.add((phys_id, v))
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        usable = os.cpu_count()
    return {"cpu_model": model, "physical_cores": len(pairs) or None, "logical_cpus": logical or os.cpu_count(),
            "usable_cpus": usable}


def cpu_quota():
    """CPUs this job may use by its cgroup quota (cgroup v2 cpu.max / v1 cfs_quota_us), or None when
    unlimited or unreadable: the GPU boxes give one GPU's job a share of the host's cores this way
    (their affinity mask still lists every CPU)."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()[:2]
        if q != "max":
            return max(1, int(int(q) / int(per)))
        return None
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as fh:
            q = int(fh.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as fh:
            per = int(fh.read())
        return max(1, int(q / per)) if q > 0 else None
    except (OSError, ValueError):
        return None


def omp_threads_env():
    """OMP_NUM_THREADS as an int (its first entry, OpenMP's nested-list syntax '8,4' allowed), or None
    when unset or malformed — recorded, never used to choose the CPU baseline's thread count."""
    v = os.environ.get("OMP_NUM_THREADS", "")
    try:
        n = int(v.split(",")[0])
        return n if n > 0 else None
    except ValueError:
        return None


def cpu_threads():
    """Threads for the CPU reference path: the CPUs this job may actually use — the cgroup CPU quota
    when there is one (the GPU boxes give one GPU's job 16 of the host's 128 physical cores this way;
    its affinity mask still lists every CPU, and 128 threads under a 16-CPU quota run throttled, 2.5x
    slower than 16), else the host's physical cores (set_num_threads(<physical
    cores>)), bounded by the CPUs this process may run on."""
    h = host_cpu()
    h["cgroup_cpu_quota"] = cpu_quota()
    h["omp_num_threads_env"] = omp_threads_env()
    n = h["physical_cores"] or h["usable_cpus"] or 1
    n = max(1, min(n, h["usable_cpus"] or n))
    if h["cgroup_cpu_quota"]:
        n = min(n, h["cgroup_cpu_quota"])
    return n, h


def cpu_baseline(args, over_batch=4):
    """cpu_baseline leg: the oracle restatement (oracle/cad_oracle.py: LibTorch CPU, the ATen kernels
    the reference dispatches; the reference source and its compiled harness stay in the build
    container) timed on this host on a bounded sample of the workload — bs`cpu_sample_batch` (32: the
    workload's own batch, BN statistics over bs32) at the benchmark resolution, 1 warm-up +
    `cpu_sample_steps` timed train steps at the job's CPU share (cpu_threads: the
    cgroup quota, the reported value).  Beside it, labelled as such: one bs`over_batch` step at all of
    the host's physical cores, which oversubscribes the quota when there is one."""
    import torch
    from oracle import cad_oracle as O
    threads, host = cpu_threads()
    B, H, W, f = args.cpu_sample_batch, args.height, args.width, args.features
    w = tuple(float(x) for x in args.weights.split(","))
    params = O.init_params(f, seed=42, model=args.model)
    bufs = O.init_buffers(f, model=args.model)
    rgb, gt, K = [torch.from_numpy(a) for a in O.synth_batch(B, H, W)]
    prev = torch.get_num_threads()
    ref = O.Trainer(params, bufs, weights=w, model=args.model)
    over = None
    try:
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        ref.step(rgb, gt, K)                      # warm-up
        warm = time.perf_counter() - t0
        # (a progress line per step: a bs32 CPU step takes ~50 s, and a run silent for minutes reads as hung)
        log(f"cpu baseline: warm-up step {warm:.1f} s")
        t0 = time.perf_counter()
        for i in range(args.cpu_sample_steps):
            ref.step(rgb, gt, K)
            log(f"cpu baseline: step {i + 1}/{args.cpu_sample_steps} at {time.perf_counter() - t0:.1f} s")
        dt = time.perf_counter() - t0
        log(f"cpu baseline: warm-up {warm:.1f} s, {args.cpu_sample_steps} steps {dt:.1f} s at {threads} threads")
        phys = host["physical_cores"] or 0
        if host["cgroup_cpu_quota"] and phys > threads and over_batch:
            torch.set_num_threads(phys)
            sub = tuple(t[:over_batch] for t in (rgb, gt, K))
            t1 = time.perf_counter()
            ref.step(*sub)
            over = {"threads": phys, "batch": over_batch, "steps": 1,
                    "images_per_s": round(over_batch / (time.perf_counter() - t1), 4),
                    "note": (f"all {phys} physical cores under the job's {host['cgroup_cpu_quota']}-CPU cgroup quota: "
                             f"oversubscribed (throttled), not the baseline; one bs{over_batch} step, no own warm-up")}
    finally:
        torch.set_num_threads(prev)
    return {"value": round(B * args.cpu_sample_steps / dt, 4), "unit": "images/s", "cores": threads, "kind": "port",
            "sample": (f"{args.model} bs{B} {H}x{W} f={f} loss weights {args.weights}, fp32 (the reference's only "
                       f"precision), 1 warm-up + {args.cpu_sample_steps} timed train steps of the oracle restatement "
                       f"(oracle/cad_oracle.py on LibTorch CPU) at {threads} threads = "
                       + (f"the job's cgroup CPU quota (one GPU's share of the host's {host['physical_cores']} "
                          f"physical cores)" if host["cgroup_cpu_quota"] else "the host's physical cores")
                       + " (BASELINE.md §3)"),
            "seconds": round(dt, 2), "warmup_seconds": round(warm, 2),
            "oversubscribed_all_cores": over, "host": host}


def parity_steps(args, cad, dev, steps=10, B=2):
    """SURVEY §8(d) / BASELINE.md §3: `steps` identical train steps on the GPU (the headline's engine)
    and on the CPU reference path (oracle restatement, fp32, the job's cgroup CPU share of the host) from the same
    weights and batch (bs`B` at the benchmark resolution); after step 1 and after step `steps`:
    train-mode prediction max relative error, loss relative error, then the eval-mode prediction
    (BN running statistics) and the computeDepthMetrics abs_rel of both on a held-out batch.
    Witness: the same trajectory in fp64 (the oracle restatement evaluated by ATen's GPU kernels in
    fp64 — the exact-arithmetic yardstick), so each fp32 path's own drift from exact arithmetic is
    reported beside the GPU-vs-CPU difference: Adam's first steps move every weight by ~lr sign(g),
    so gradients whose sign sits within fp32 rounding of zero move weights apart on ANY two fp32 paths
    and the trajectories separate; `drift_ratio` = GPU drift / CPU-path drift from fp64."""
    import torch
    from oracle import cad_oracle as O
    threads, host = cpu_threads()
    threads = min(threads, host["cgroup_cpu_quota"] or threads)   # a correctness check: the job's CPU share
    H, W, f = args.height, args.width, args.features
    w = tuple(float(x) for x in args.weights.split(","))
    params = O.init_params(f, seed=42, model=args.model)
    bufs = O.init_buffers(f, model=args.model)
    rgb, gt, K = [torch.from_numpy(a) for a in O.synth_batch(B, H, W)]
    hr, hg, hk = [torch.from_numpy(a) for a in O.synth_batch(2, H, W, rgb_seed=0xBEEF, hole_seed=0xF00D)]
    cls = {"baseline": cad.BaselineUNet, "film": cad.IntrinsicsConditionedUNet,
           "rayfilm": cad.RayConditionedUNet}[args.model]
    model = cls(3, f, max_depth=10.0, batch=B, height=H, width=W, device=dev.index)
    st = dict(params)
    st.update(bufs)
    model.load_state_dict(st)
    loss = cad.CombinedDepthLoss(*w, batch=B, height=H, width=W, device=dev.index)
    tr = cad.Trainer(model, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
    rg, gg, kg = rgb.to(dev), gt.to(dev), K.to(dev)
    hrg, hgg, hkg = hr.to(dev), hg.to(dev), hk.to(dev)
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    ref = O.Trainer(params, bufs, weights=w, model=args.model)
    ref64 = O.Trainer(params, bufs, weights=w, model=args.model, dtype=torch.float64, device=dev)

    def mre(a, b):
        den = b.abs().max().item()
        return (a.double() - b.double()).abs().max().item() / (den if den > 0 else 1.0)
    out = {"what": (f"{steps} identical train steps on the GPU ({args.dtype} engine) and on the CPU reference path "
                    f"(fp32, {threads} threads) from the same weights and bs{B} {H}x{W} batch; after step 1 and step "
                    f"{steps}: train-mode prediction, loss, then eval-mode forward + computeDepthMetrics abs_rel on a "
                    f"held-out bs2 batch; fp64_witness: both paths' distance from the same trajectory in fp64 "
                    f"(the restatement on ATen's GPU kernels)")}
    try:
        for k in range(1, steps + 1):
            gl = tr.train_step(rg, gg, kg)[0].item()
            r = ref.step(rgb, gt, K)
            r64 = ref64.step(rgb, gt, K)
            log(f"parity: step {k}/{steps}")
            if k in (1, steps):
                model.eval()
                g_eval = (model(hrg, cad.camera_from_K(hkg)) if model.conditioned else model(hrg))
                g_abs = cad.depth_metrics(g_eval, hgg)["abs_rel"]
                model.train()
                c_eval = ref.predict_eval(hr, hk if args.model != "baseline" else None)
                c_abs = O.abs_rel_per_sample(c_eval, hg)
                e64 = ref64.predict_eval(hr, hk if args.model != "baseline" else None).cpu()
                p64 = r64["pred"].cpu()
                gpu64, cpu64 = mre(tr.pred.cpu(), p64), mre(r["pred"], p64)
                out[f"after_step_{k}"] = {
                    "pred_max_rel_err": mre(tr.pred.cpu(), r["pred"]),
                    "loss_rel_err": abs(gl - r["loss"]) / abs(r["loss"]),
                    "eval_pred_max_rel_err": mre(g_eval.cpu(), c_eval),
                    "abs_rel_gpu": round(g_abs, 6), "abs_rel_cpu_ref": round(c_abs, 6),
                    "abs_rel_delta": abs(g_abs - c_abs),
                    "fp64_witness": {
                        "pred_gpu_vs_fp64": gpu64, "pred_cpu_ref_vs_fp64": cpu64,
                        "eval_pred_gpu_vs_fp64": mre(g_eval.cpu(), e64), "eval_pred_cpu_ref_vs_fp64": mre(c_eval, e64),
                        "drift_ratio": gpu64 / cpu64 if cpu64 > 0 else None}}
    finally:
        torch.set_num_threads(prev)
        del tr, loss, model, ref64
        torch.cuda.empty_cache()
    return out


def profiled(lib, only=None):
    """Context of a region whose kernels libcad times with HIP events on their launch streams
    (csrc/host/profiler.cpp); yields a callable returning the per-kernel report.  only: time just the
    launches of that kernel (the timed region brackets only the kernel whose roofline it reports:
    events around every GEMM launch cost ~2 % of a configs[3] step)."""
    import contextlib

    if os.environ.get("CAD_BENCH_EVENTS") == "all":   # A/B: events around every GEMM launch
        only = None

    @contextlib.contextmanager
    def cm():
        lib.cad_profile_reset()
        lib.cad_profile_only(only.encode() if only else None)
        lib.cad_profile_enable(1)
        box = {}
        try:
            yield lambda: box.get("prof", [])
        finally:
            lib.cad_profile_enable(0)
            lib.cad_profile_only(None)
            n = lib.cad_profile_report(None, 0)
            buf = C.create_string_buffer(n)
            lib.cad_profile_report(buf, n)
            box["prof"] = json.loads(buf.value.decode())
    return cm()


def gemm_census(lib, step, dev, steps=1):
    """An untimed pass of `steps` steps with every GEMM launch timed: names the dominant kernel (the
    largest total time) whose launches the timed region then brackets, and gives the per-step GEMM
    summary (all_gemm_kernels)."""
    import torch
    # every GEMM alone: the S3 engine's weight gradients otherwise run on a second stream beside the
    # dgrad chain (cad_api.cpp wgrad_stream), where a launch's duration includes sharing the CUs
    prev = os.environ.get("CAD_SIDE_WGRAD")
    os.environ["CAD_SIDE_WGRAD"] = "0"
    try:
        with profiled(lib) as prof:
            for _ in range(steps):
                step()
            torch.cuda.synchronize(dev)
    finally:
        if prev is None:
            del os.environ["CAD_SIDE_WGRAD"]
        else:
            os.environ["CAD_SIDE_WGRAD"] = prev
    return prof()


def dominant_name(census):
    gemm = [r for r in census if r["gflop"] > 0]
    return max(gemm, key=lambda r: r["ms"])["name"] if gemm else None


def roofline_of(prof, steps, ms_per_step, show=False, table="pmc_traffic.json", census=None, census_steps=1):
    """roofline object of the dominant MFMA kernel (largest total time) of a profiled region:
    achieved = its algorithmic FLOPs / its summed HIP-event durations, against its engine's ceiling.
    census: the untimed every-GEMM pass (gemm_census) that named the kernel `prof` (the timed region,
    events around that kernel only) timed; the GEMM summary then comes from the census."""
    every = census if census is not None else prof
    esteps = census_steps if census is not None else steps
    if show:
        for r in sorted(every, key=lambda r: -r["ms"])[:24]:
            log(f"  {r['ms'] / esteps:8.2f} ms/step  {r['gflop'] / r['ms'] if r['ms'] else 0:7.2f} TF/s  "
                f"x{r['launches'] // esteps:<3d} {r['name']}")
    gemm = [r for r in every if r["gflop"] > 0]   # (split-K reductions are profiled at 0 FLOP)
    if not gemm:
        return None
    dom = max(gemm, key=lambda r: r["ms"])
    timed = [r for r in prof if r["name"] == dom["name"] and r["ms"] > 0]
    from_timed = census is None or bool(timed)
    solo = dom if census is not None else None
    if census is not None and timed:
        dom = timed[0]   # the timed region's own launches of that kernel
    dsteps = steps if from_timed else esteps
    achieved = dom["gflop"] / dom["ms"]   # GFLOP/ms == TFLOP/s
    # k_<op>[_win]_<engine>[p]: engine s3 / bf16 / none (f32); p = pre-split operands
    kname = re.search(r"(k_\w+)", dom["name"]).group(1)
    s3 = kname.endswith("_s3")
    b1 = kname.endswith(("_bf16", "_bf16p", "_bf16p4", "_bf16d"))
    x8 = kname.endswith("_x8")
    peak = (S3_PEAK_TFLOPS if s3 else BF16_MFMA_PEAK_TFLOPS if b1 else MX8_MFMA_PEAK_TFLOPS if x8
            else FP32_MFMA_PEAK_TFLOPS)
    roof = {"bound": "mfma", "achieved": round(achieved, 3), "peak": round(peak, 1), "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": pmc_traffic(dom["name"], table),
            "arith": ("fp32 via exact 3-way bf16 split, 6 bf16 MFMA products per fp32 MAC: peak = dense "
                      "bf16 MFMA 2516.6 / 6; achieved counts algorithmic fp32 FLOPs") if s3 else
                     ("bf16 operands, fp32 accumulation (v_mfma_f32_32x32x16_bf16): peak = dense bf16 MFMA")
                     if b1 else
                     ("MXFP8 E4M3 operands, one E8M0 scale per 32 k, fp32 accumulation "
                      "(v_mfma_scale_f32_32x32x64_f8f6f4): peak = 2 x dense bf16") if x8 else
                     "fp32 MFMA (v_mfma_f32_32x32x2_f32)",
            "kernel": dom["name"], "launches_per_step": dom["launches"] // dsteps,
            "avg_launch_ms": round(dom["ms"] / dom["launches"], 4),
            "gflop_per_launch": round(dom["gflop"] / dom["launches"], 3)}
    roof["timed_in"] = ("the timed region (HIP events around this kernel's launches only)" if from_timed
                        else "the census step")
    if solo is not None and solo is not dom and solo["ms"] > 0:
        sa = solo["gflop"] / solo["ms"]
        roof["solo"] = {"achieved": round(sa, 3), "frac": round(sa / peak, 4),
                        "avg_launch_ms": round(solo["ms"] / solo["launches"], 4),
                        "from": "the untimed census step, every GEMM launch alone on the step's stream"}
        if sa > 1.2 * achieved:
            roof["co_running"] = ("in the timed region this kernel runs on a second stream beside the dgrad "
                                  "chain (the step is ~2 % faster for it): its launches share the CUs, so "
                                  "their durations exceed the solo ones; frac above is per launch as timed")
    tot_ms = sum(r["ms"] for r in gemm)
    tot_gf = sum(r["gflop"] for r in gemm)
    roof["all_gemm_kernels"] = {"tflops": round(tot_gf / tot_ms, 3), "ms_per_step": round(tot_ms / esteps, 3),
                                "share_of_step": round(tot_ms / esteps / ms_per_step, 4),
                                "from": "an untimed census step, every GEMM launch timed" if census is not None
                                else "the timed region"}
    return roof


def flop_per_image(f=64, H=480, W=640):
    """Algorithmic FLOPs of one trained image through BaselineUNet(3, f) (forward + dgrad +
    wgrad of every conv / ConvT / the head; enc1.conv1 has no dgrad, its input is the image):
    1,353.646 GFLOP at f = 64, 3,044.023 at f = 96 (train_config_production.yaml)."""
    P = lambda l: (H >> l) * (W >> l)
    t = 2 * 2 * P(0) * f * 27 + 3 * 2 * P(0) * f * 9 * f + 3 * 2 * P(0) * f
    for l in range(1, 5):          # enc2..enc4, bottleneck: C/2 -> C, C -> C
        C = f << l
        t += 3 * (2 * P(l) * C * 9 * C // 2 + 2 * P(l) * C * 9 * C)
    for l in range(4):             # dec: ConvT 2C -> C (2x2/s2), conv1 cat 2C -> C, conv2 C -> C
        C = f << l
        t += 3 * (2 * P(l) * 2 * C * C + 2 * P(l) * C * 9 * 2 * C + 2 * P(l) * C * 9 * C)
    return float(t)


def extra_leg(cad, lib, dev, config, steps=10, warmup=3, B=32, H=480, W=640, f=64):
    """A bounded measurement of another BASELINE workload in the same run (driver-observed):
    configs[2] (ray+FiLM U-Net, bf16 GEMMs, full loss) or configs[3]'s per-GPU step (baseline_unet,
    bf16 GEMMs, full loss), with the roofline of its dominant kernel."""
    import torch
    from cad_amd import synthetic
    model_name, dtype = PRESETS[config]
    prev = lib.cad_get_gemm_engine()
    assert lib.cad_set_gemm_engine(2 if dtype == "bf16" else 1) == 0
    try:
        cls = {"baseline": cad.BaselineUNet, "rayfilm": cad.RayConditionedUNet}[model_name]
        model = cls(3, f, max_depth=10.0, batch=B, height=H, width=W, device=dev.index)
        lw = (1.0, 0.0, 0.0, 0.0) if config == 2 else (1.0, 0.1, 0.001, 0.01)
        loss = cad.CombinedDepthLoss(*lw, batch=B, height=H, width=W, device=dev.index)
        tr = cad.Trainer(model, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0)
        rgb, gt, K = (t.to(dev) for t in synthetic.device_batch(B, H, W, "cpu"))
        for _ in range(warmup):
            tr.train_step(rgb, gt, K)
        census = gemm_census(lib, lambda: tr.train_step(rgb, gt, K), dev)
        with profiled(lib, dominant_name(census)) as prof:
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_step(rgb, gt, K)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
        last = tr.loss5[0].item()
        del tr, loss, model
        torch.cuda.empty_cache()
    finally:
        lib.cad_set_gemm_engine(prev)
    value = B * steps / dt
    wl = WORKLOADS[config] if f == 64 else (
        f"baseline_unet f={f} (train_config_production.yaml: init_features 96) train step, bs{B}/GPU {H}x{W} "
        f"{dtype} GEMMs, " + ("SI-only loss" if config == 2 else "full loss"))
    out = {"workload": wl, "value": round(value, 3), "unit": "images/s", "init_features": f,
           "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps, "warmup": warmup, "dtype": dtype,
           "last_loss": last, "roofline": roofline_of(prof(), steps, 1e3 * dt / steps, census=census)}
    if model_name == "baseline" and (H, W) == (480, 640):
        fl = flop_per_image(f, H, W)
        out["step_tflops_algorithmic"] = round(fl * value / 1e12, 3)
        out["mfma_frac_dense_bf16"] = round(fl * value / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4)
        if dtype == "fp32":
            out["mfma_frac_s3_ceiling"] = round(fl * value / 1e12 / S3_PEAK_TFLOPS, 4)
    return out


def resunet_macs_per_image(H=480, W=640):
    """Forward multiply-accumulates of one image through the config-5 network (resunet.cpp layout),
    and how many of them have a dgrad (all but the stem conv, whose input is the image)."""
    macs = 0
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    stem = h * w * 64 * 3 * 49
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cin = 64
    for L, (wd, n) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3))):
        for i in range(n):
            s = 2 if (L > 0 and i == 0) else 1
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            macs += h * w * cin * wd + ho * wo * (wd * 9 * wd + wd * 4 * wd)
            if i == 0:
                macs += ho * wo * cin * 4 * wd
            cin, h, w = 4 * wd, ho, wo
    for l, cu, C, sk in ((4, 2048, 512, 1024), (3, 512, 256, 512), (2, 256, 128, 256), (1, 128, 64, 64), (0, 64, 32, 0)):
        hh, ww = H >> l, W >> l
        macs += (hh // 2) * (ww // 2) * cu * 4 * C + hh * ww * (sk + C) * 9 * C + hh * ww * C * 9 * C
    macs += H * W * 32
    return stem + macs, macs


def extra_leg_resunet(cad, lib, dev, steps=10, warmup=3, B=32, H=480, W=640, fp8=False):
    """configs[4]'s per-GPU step: ResNet-50 encoder + U-Net decoder (resunet.cpp), bs32 480x640, full
    loss, bf16 contraction operands; fp8=True: the forward conv-GEMMs on MXFP8 E4M3 operands
    (cad_resunet_set_fp8, the "fp8 MFMA conv-GEMM" configs[4] names)."""
    import torch
    from cad_amd import synthetic
    model = cad.ResNetUNet(batch=B, height=H, width=W, device=dev.index, fp8=fp8)
    loss = cad.CombinedDepthLoss(1.0, 0.1, 0.001, 0.01, batch=B, height=H, width=W, device=dev.index)
    rgb, gt, K = (t.to(dev) for t in synthetic.device_batch(B, H, W, "cpu"))
    pred = torch.empty((B, 1, H, W), device=dev)
    dpred, loss5 = torch.empty_like(pred), torch.zeros(5, device=dev)
    for _ in range(warmup):
        model.train_step(loss, rgb, gt, K, pred=pred, dpred=dpred, loss5=loss5)
    census = gemm_census(lib, lambda: model.train_step(loss, rgb, gt, K, pred=pred, dpred=dpred, loss5=loss5), dev)
    with profiled(lib, dominant_name(census)) as prof:
        t0 = time.perf_counter()
        for _ in range(steps):
            model.train_step(loss, rgb, gt, K, pred=pred, dpred=dpred, loss5=loss5)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
    last = loss5[0].item()
    params = model.count_parameters()
    model_fp8_units = model.fp8_units if fp8 else 0
    del model, loss
    torch.cuda.empty_cache()
    value = B * steps / dt
    fwd, with_dgrad = resunet_macs_per_image(H, W)
    flop_img = 2 * (2 * fwd + with_dgrad)   # forward + wgrad of every conv, dgrad of all but the stem
    return {"workload": "ResNet-50 encoder + U-Net decoder train step, configs[4] per-GPU: bs32 480x640, "
                        + ("forward conv-GEMMs on MXFP8 E4M3 operands (backward bf16)" if fp8 else
                           "bf16 GEMM operands") + ", full loss",
            "fp8_units": model_fp8_units,
            "value": round(value, 3), "unit": "images/s", "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps,
            "warmup": warmup, "dtype": "fp8+bf16" if fp8 else "bf16", "params": params, "last_loss": last,
            "gflop_per_image": round(flop_img / 1e9, 2),
            "mfma_frac_dense_bf16": round(flop_img * value / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4),
            "roofline": roofline_of(prof(), steps, 1e3 * dt / steps, table="pmc_traffic_c5.json", census=census)}


def extra_leg_geonet(cad, lib, dev, steps=3, warmup=2, B=8, H=480, W=640, f=64):
    """The geometry-aware family (no BASELINE config names it): one
    GeometryAwareNetwork(3, 64, 4, 10, use_pcl, use_attention) train step at 480x640 on the fp32 (S3)
    engine, full loss, bs8 (its six-level activations with CBAM / PCL state are ~4x the U-Net's)."""
    import torch
    from cad_amd import synthetic
    prev = lib.cad_get_gemm_engine()
    lib.cad_set_gemm_engine(1)
    try:
        model = cad.GeometryAwareNetwork(3, f, 4, 10.0, batch=B, height=H, width=W, device=dev.index)
        loss = cad.CombinedDepthLoss(1.0, 0.1, 0.001, 0.01, batch=B, height=H, width=W, device=dev.index)
        rgb, gt, K = (t.to(dev) for t in synthetic.device_batch(B, H, W, "cpu"))
        rays = cad.ray_directions(K, H, W)
        pred = torch.empty((B, 1, H, W), device=dev)
        dpred, loss5 = torch.empty_like(pred), torch.zeros(5, device=dev)
        for _ in range(warmup):
            model.train_step(loss, rgb, gt, K, rays=rays, pred=pred, dpred=dpred, loss5=loss5)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            model.train_step(loss, rgb, gt, K, rays=rays, pred=pred, dpred=dpred, loss5=loss5)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        last = loss5[0].item()
        params = model.count_parameters()
        del model, loss
        torch.cuda.empty_cache()
    finally:
        lib.cad_set_gemm_engine(prev)
    return {"workload": f"GeometryAwareNetwork(3, {f}) train step (CBAM + PCL, six levels): bs{B} {H}x{W} "
                        "fp32 (S3) GEMMs, full loss",
            "value": round(B * steps / dt, 3), "unit": "images/s", "ms_per_step": round(1e3 * dt / steps, 3),
            "steps": steps, "warmup": warmup, "dtype": "fp32", "params": params, "last_loss": last}


def pmc_traffic(kernel_name, table="pmc_traffic.json"):
    """HBM bytes per launch of `kernel_name` from the committed rocprofv3 PMC summary, if any
    (profiles/pmc_traffic.json: the U-Net workloads; pmc_traffic_c5.json: configs[4]'s network, whose
    kernels share names with the U-Net's at other shapes)."""
    path = os.path.join(ROOT, "profiles", table)
    try:
        with open(path) as fh:
            d = json.load(fh)
        # rocprofv3 prints a non-template kernel without its "void " return type
        for k in (kernel_name, kernel_name[5:] if kernel_name.startswith("void ") else None):
            if k and k in d:
                return d[k].get("hbm_bytes_per_launch")
        return None
    except Exception:
        return None


def data_path(cad, dev, B, H, W, h0=530, w0=730, reps=10):
    """Device batch assembly (cad_batcher_assemble: SunRGBDLoader resize + train augmentation) of a
    bs-B batch of decoded 530x730 SUN RGB-D-sized samples (u8 rgb, u16 depth) with the loader's
    default augmentation draws; measured apart from the step (the headline excludes data loading).
    Algorithmic bytes per image: source rgb + depth read once, fp32 rgb + depth written, plus the
    stage-1 planes written and read back for the augmented second resize."""
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    sampler = cad.AugSampler(42)
    K = np.array([[518.858, 0, 325.582], [0, 519.470, 253.736], [0, 0, 1]], dtype=np.float32)
    samples = []
    for _ in range(B):
        s = {"rgb": torch.from_numpy(rng.integers(0, 256, (h0, w0, 3), dtype=np.uint8)).to(dev),
             "depth": torch.from_numpy(rng.integers(0, 12000, (h0, w0), dtype=np.int16)).to(dev), "K": K, "bgr": 1}
        s.update(sampler.draw(H, W))
        samples.append(s)
    asm = cad.BatchAssembler(B, H, W, device=dev.index)
    out = asm.assemble(samples)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        asm.assemble(samples, out=out)
    e1.record()
    torch.cuda.synchronize(dev)
    ms = e0.elapsed_time(e1) / reps
    per_img = h0 * w0 * 5 + H * W * 16 + H * W * 16 * 2
    return {"what": f"device batch assembly (resize + crop/flip/jitter + resize) of bs{B} decoded {h0}x{w0} "
                    f"samples to {H}x{W}", "ms_per_batch": round(ms, 4), "images_per_s": round(B / ms * 1e3, 1),
            "achieved_GBps": round(per_img * B / ms / 1e6, 1), "peak_GBps": HBM_PEAK_GBS}


DUMP_PRED_ELEMS = 12 << 20    # 48 MiB of float32: the headline's (32, 1, 480, 640) prediction fits whole
DUMP_PARAM_ELEMS = 1 << 20    # 4 MiB: a sample of the 31 M updated parameters
DUMP_SEED = 0x5EED


def dump_sample(a, limit):
    """`a` whole when it has at most `limit` elements, else a fixed sample of it: `limit` sorted flat
    indices drawn (with replacement) from default_rng(DUMP_SEED), the same for every run of one shape."""
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.size <= limit:
        return a
    idx = np.sort(np.random.default_rng(DUMP_SEED).integers(0, a.size, size=limit))
    return a.reshape(-1)[idx]


def dump_outputs(dirpath, trainer, model):
    """--dump-outputs: what the last timed train step handed its caller, one float32 DIR/<name>.npy each
    (under 64 MB in all), so that two builds run with the same arguments (the synthetic batch and
    the initial weights are fixed streams) can be compared output for output:
      pred         the step's train-mode prediction (B, 1, H, W) (Trainer.pred)
      loss5        total, si, grad, smooth, reproj of that prediction (train_step's return value)
      grad_norm    the gradient norm clip_grad_norm_ measured in that step
      params       the parameters after that step's Adam update, named_parameters() order, flattened
                   (a seeded sample of DUMP_PARAM_ELEMS of them)."""
    import numpy as np
    import torch
    torch.cuda.synchronize(model.device)
    os.makedirs(dirpath, exist_ok=True)
    params = np.concatenate([v.numpy().reshape(-1) for v in model.named_parameters().values()])
    arrays = {"pred": dump_sample(trainer.pred.cpu().numpy(), DUMP_PRED_ELEMS),
              "loss5": dump_sample(trainer.loss5.cpu().numpy(), 5),
              "grad_norm": np.array([model.last_grad_norm()], dtype=np.float32),
              "params": dump_sample(params, DUMP_PARAM_ELEMS)}
    for name, a in arrays.items():
        np.save(os.path.join(dirpath, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def setup_dist(args):
    """N>1: one rank per GPU.  torch.distributed (gloo, host memory only) is the launcher's store and
    the host-side barrier / max-over-ranks clock; the gradient exchange itself is libcad's RCCL
    communicator (cad_comm_*, cad_unet_backward_allreduce) — the path build/train uses — created from
    rank 0's unique id handed over through that store.  --exchange torch selects the torch.distributed
    bucketed path instead (the only one that runs when several ranks share one GPU: CAD_BENCH_DEVICE)."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE")
    # CAD_BENCH_DEVICE: rehearsal of the N>1 path on a 1-GPU box (every rank on one device) — never set
    # for the driver's runs (one rank per GPU)
    local = int(os.environ.get("CAD_BENCH_DEVICE", local))
    if world > 1:
        dist.init_process_group("gloo")
    return world, rank, local


def rccl_unique_id(cad, rank):
    """Rank 0's 128-byte RCCL unique id (cad_comm_get_unique_id: host-side bootstrap, no GPU call),
    handed to every rank through the launcher's gloo store (tests/test_bench_dist.py covers it on CPU)."""
    import torch.distributed as dist
    obj = [cad.Communicator.unique_id() if rank == 0 else None]
    dist.broadcast_object_list(obj, src=0)
    uid = obj[0]
    if not isinstance(uid, bytes) or len(uid) != 128:
        raise RuntimeError(f"rank {rank}: bad RCCL unique id from rank 0 ({type(uid).__name__})")
    return uid


def timed_region(step, steps, warmup, world, dev):
    """W untimed warm-up steps, then exactly `steps` steps bracketed by a barrier + synchronize on
    both sides; the max over ranks of the elapsed wall time."""
    import torch
    import torch.distributed as dist
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize(dev)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    return elapsed


def exchange_report(xs, steps, world):
    """Per-step gradient-exchange accounting of a timed region (Trainer / ResNetUNet exchange_stats):
    the communicator's rank count, all-reduces and bytes per step, and the exposed exchange time
    (compute stream idle between its last backward kernel and the release by the last all-reduce)
    as the mean over timed steps, max over ranks."""
    import torch
    import torch.distributed as dist
    ex = xs["exposed_ms"] / xs["timed_calls"] if xs.get("timed_calls") else None
    sp = xs["span_ms"] / xs["timed_calls"] if xs.get("timed_calls") and xs.get("span_ms") is not None else None
    ex_max = ex
    if world > 1 and ex is not None:
        t = torch.tensor([ex], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ex_max = t.item()
    return {"backend": xs.get("backend"), "comm_size": xs.get("comm_size"),
            "steps_accounted": xs.get("calls"), "allreduces_per_step": xs["buckets"] / max(1, xs["calls"]),
            "bytes_allreduced_per_step": xs["bytes"] // max(1, xs["calls"]),
            "exposed_ms_per_step_rank0": None if ex is None else round(ex, 4),
            "exposed_ms_per_step_max_rank": None if ex_max is None else round(ex_max, 4),
            "allreduce_span_ms_per_step_rank0": None if sp is None else round(sp, 4)}


def dp_leg(cad, lib, dev, world, rank, comm, pg, config=4, steps=10, warmup=3, B=32, H=480, W=640, f=64):
    """A BASELINE DP workload at N = world ranks with the job's gradient exchange: configs[3]
    (config=4: baseline_unet, bf16 GEMMs, full loss, bs32 per GPU -> global bs32*N) or configs[4]
    (config=5: ResNet-50 encoder + U-Net decoder, bf16; fp8=True: MXFP8 forward conv-GEMMs).
    Every rank runs it (collectives); rank 0 reports whole-job images/s over the max-over-ranks clock
    and the exchange accounting."""
    import torch
    import torch.distributed as dist
    from cad_amd import synthetic
    fp8 = config == "5x8"
    prev = lib.cad_get_gemm_engine()
    assert lib.cad_set_gemm_engine(2) == 0
    try:
        if config == 4:
            model = cad.BaselineUNet(3, f, max_depth=10.0, batch=B, height=H, width=W, device=dev.index)
        else:
            model = cad.ResNetUNet(batch=B, height=H, width=W, device=dev.index, fp8=fp8)
        if comm is not None:
            comm.broadcast_parameters(model, 0)
        elif pg is not None:
            dist.broadcast(model.flat_params, 0, group=pg)
        loss = cad.CombinedDepthLoss(1.0, 0.1, 0.001, 0.01, batch=B, height=H, width=W, device=dev.index)
        rgb, gt, K = (torch.roll(t, shifts=rank, dims=0).contiguous().to(dev)
                      for t in synthetic.device_batch(B, H, W, "cpu"))
        if config == 4:
            tr = cad.Trainer(model, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0, process_group=pg,
                             communicator=comm)
            tr.set_exchange_timing(True)
            step = lambda: tr.train_step(rgb, gt, K)
            stats = tr.exchange_stats
            last = lambda: tr.loss5[0].item()
        else:
            pred = torch.empty((B, 1, H, W), device=dev)
            dpred, loss5 = torch.empty_like(pred), torch.zeros(5, device=dev)
            if comm is not None:
                comm.set_timing(True)
                stats = lambda: dict(comm.stats(), backend="libcad RCCL communicator", comm_size=comm.size())
            else:
                model.exchange_accounting(True)
                stats = model.exchange_stats
            step = lambda: model.train_step(loss, rgb, gt, K, pred=pred, dpred=dpred, loss5=loss5,
                                            process_group=pg, communicator=comm)
            last = lambda: loss5[0].item()
        for _ in range(warmup):
            step()
        stats()   # warm-up steps are not accounted
        elapsed = timed_region(step, steps, 0, world, dev)
        xs = exchange_report(stats(), steps, world)
        out = {"workload": (WORKLOADS_DP[config] + f", DP over {world} ranks (global bs{B * world})"),
               "value": round(B * world * steps / elapsed, 3), "unit": "images/s", "n_gpus": world,
               "ms_per_step": round(1e3 * elapsed / steps, 3), "steps": steps, "warmup": warmup,
               "dtype": "fp8+bf16" if fp8 else "bf16", "last_loss": last(), "exchange": xs}
        if comm is not None:
            comm.set_timing(False)
            comm.stats()
        return out
    finally:
        lib.cad_set_gemm_engine(prev)


WORKLOADS_DP = {4: "baseline_unet train step, configs[3]: bs32/GPU 480x640 bf16 GEMMs, full loss",
                5: "ResNet-50 encoder + U-Net decoder train step, configs[4]: bs32/GPU 480x640 bf16 GEMM operands, "
                   "full loss",
                "5x8": "ResNet-50 encoder + U-Net decoder train step, configs[4]: bs32/GPU 480x640, forward "
                       "conv-GEMMs on MXFP8 E4M3 operands (backward bf16), full loss"}


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    world, rank, local = setup_dist(args)
    import cad_pkg
    cad = cad_pkg.load()
    comm, pg = None, None
    if world > 1:
        if args.exchange == "rccl":
            uid = rccl_unique_id(cad, rank)
            torch.cuda.set_device(local)
            comm = cad.Communicator(uid, world, rank, device=local)
        else:
            torch.cuda.set_device(local)
            pg = dist.new_group(backend=os.environ.get("CAD_DIST_BACKEND", "nccl"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from cad_amd import synthetic
    B, H, W, f = args.batch, args.height, args.width, args.features
    w = tuple(float(x) for x in args.weights.split(","))
    lib = cad.load_library()
    assert lib.cad_set_gemm_engine(2 if args.dtype == "bf16" else 1) == 0   # CAD_GEMM_BF16 / CAD_GEMM_S3
    cls = {"baseline": cad.BaselineUNet, "film": cad.IntrinsicsConditionedUNet,
           "rayfilm": cad.RayConditionedUNet}[args.model]
    model = cls(3, f, max_depth=10.0, batch=B, height=H, width=W, device=local)
    params_count = model.count_parameters()
    if comm is not None:
        comm.broadcast_parameters(model, 0)        # identical replicas (DDP semantics)
    elif pg is not None:
        dist.broadcast(model.flat_params, 0, group=pg)
    loss = cad.CombinedDepthLoss(*w, batch=B, height=H, width=W, device=local)
    trainer = cad.Trainer(model, loss, lr=1e-4, weight_decay=1e-5, grad_clip=1.0, process_group=pg,
                          communicator=comm)
    rgb, gt, K = (t.to(dev) for t in synthetic.device_batch(B, H, W, "cpu"))
    if world > 1:   # each replica sees its own shard of the global batch
        rgb = torch.roll(rgb, shifts=rank, dims=0).contiguous()
        gt = torch.roll(gt, shifts=rank, dims=0).contiguous()
        K = torch.roll(K, shifts=rank, dims=0).contiguous()

    if world > 1:
        trainer.set_exchange_timing(True)
    for i in range(args.warmup):
        trainer.train_step(rgb, gt, K)
    # --full: one more untimed step with every GEMM launch timed names the dominant kernel; the timed
    # region then brackets only that kernel's launches with events (every rank runs it: collectives)
    census = gemm_census(lib, lambda: trainer.train_step(rgb, gt, K), dev) if args.full else None
    xstats = trainer.exchange_stats if world > 1 else None
    if xstats:
        xstats()   # warm-up and census steps are not accounted
    if args.full:
        with profiled(lib, dominant_name(census)) as prof:
            elapsed = timed_region(lambda: trainer.train_step(rgb, gt, K), args.steps, 0, world, dev)
    else:
        elapsed = timed_region(lambda: trainer.train_step(rgb, gt, K), args.steps, 0, world, dev)
    exchange = exchange_report(xstats(), args.steps, world) if xstats else None
    last_loss = trainer.loss5[0].item()
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, trainer, model)
    dp_legs = None
    if world > 1 and args.full and not args.no_extra:
        # the DP workloads BASELINE names for the multi-GPU runs (configs[3], configs[4]) with the same
        # exchange; every rank runs them, rank 0 reports
        del trainer, loss, model
        torch.cuda.empty_cache()
        dp_legs = {}
        for key, cfg in (("config4", 4), ("config5", 5), ("config5_fp8", "5x8")):
            try:
                dp_legs[key] = dp_leg(cad, lib, dev, world, rank, comm, pg, config=cfg, B=B, H=H, W=W, f=f)
                if rank == 0:
                    log(f"DP leg {key}: {dp_legs[key]}")
            except Exception as e:   # a failing leg must not hang the others: ranks fail alike (same code)
                log(f"rank {rank}: DP leg {key} failed: {e}")
                dp_legs[key] = {"error": str(e)[:500]}
            gc.collect()   # the leg's model and arena go before the next one is created
            torch.cuda.empty_cache()

    if rank == 0:
        images = B * world * args.steps
        value = images / elapsed
        ms_per_step = 1e3 * elapsed / args.steps
        roof = roofline_of(prof(), args.steps, ms_per_step, show=True, census=census) if args.full else None
        step_tflops = (FLOP_PER_IMAGE_480x640_F64 * value / 1e12
                       if (H, W, f, args.model) == (480, 640, 64, "baseline") else None)
        dp, extra, cpu, parity = None, None, None, None
        if dp_legs is None:
            del trainer, loss, model
            torch.cuda.empty_cache()
        if world == 1 and args.full and not args.no_extra:
            extra = {}
            for cfg in (3, 4):
                if cfg == args.config:
                    continue
                try:
                    extra[f"config{cfg}"] = extra_leg(cad, lib, dev, cfg)
                    log(f"extra leg config {cfg}: {extra[f'config{cfg}']}")
                except Exception as e:
                    log(f"extra leg config {cfg} failed: {e}")
            for cfg in (2, 4):   # the reference's production width (train_config_production.yaml:26-27)
                key = f"config{cfg}_f96"
                try:
                    extra[key] = extra_leg(cad, lib, dev, cfg, f=96)
                    log(f"extra leg {key}: {extra[key]}")
                except Exception as e:
                    log(f"extra leg {key} failed: {e}")
            for key, fp8 in (("config5", False), ("config5_fp8", True)):
                try:
                    extra[key] = extra_leg_resunet(cad, lib, dev, fp8=fp8)
                    log(f"extra leg {key}: {extra[key]}")
                except Exception as e:
                    log(f"extra leg {key} failed: {e}")
            try:
                extra["geometry"] = extra_leg_geonet(cad, lib, dev)
                log(f"extra leg geometry-aware network: {extra['geometry']}")
            except Exception as e:
                log(f"extra leg geometry-aware network failed: {e}")
            try:
                dp = data_path(cad, dev, B, H, W)
            except Exception as e:
                log(f"data-path measurement failed: {e}")
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                cpu = cpu_baseline(args)
                log(f"cpu baseline: {cpu}")
            except Exception as e:
                log(f"cpu baseline failed: {e}")
            try:
                parity = parity_steps(args, cad, dev)
                log(f"parity: {parity}")
            except Exception as e:
                log(f"parity check failed: {e}")
        out = {
            "metric": METRIC, "value": round(value, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": args.dtype, "data": "synthetic (SUN-RGB-D-shaped, HBM-resident)",
            "full": args.full, "dumped_outputs": dumped,
            "config": {"workload": WORKLOADS[args.config] if (args.model, args.dtype) == PRESETS[args.config] else
                       f"{args.model} train step, {args.dtype} GEMMs, bs{B}/GPU {H}x{W}, loss weights {args.weights}",
                       "model": args.model,
                       "global_batch": B * world, "height": H, "width": W, "init_features": f,
                       "params": params_count, "loss_weights": list(w),
                       "parallelism": f"dp{world}", "optimizer": "adam(lr1e-4,wd1e-5)+clip1.0",
                       "gradient_exchange": (None if world == 1 else
                                             "libcad RCCL communicator: decoder-first buckets overlapped with the "
                                             "backward (cad_unet_backward_allreduce)" if comm is not None else
                                             "torch.distributed bucketed all-reduce (GradBucketer)")},
            "step_tflops_algorithmic": round(step_tflops, 3) if step_tflops else None,
            "last_loss": last_loss,
            "roofline": roof,
            "cpu_baseline": cpu,
            "parity": parity,
            "bf16_workloads": extra,
            "data_path": dp,
        }
        if world > 1:
            out["exchange"] = exchange
            out["dp_workloads"] = dp_legs
        print(json.dumps(out), flush=True)
    comm = None
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
