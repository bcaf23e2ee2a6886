"""Eval-forward A/B on one box: alternate child processes of several arms — an environment (a tuning switch, or
CAD_LIB=<variant build>) and the fused eval forward on or off — so every arm sees the same box, clock and thermal
history.  Each child builds the model, runs --warmup eval-mode forwards, then times --forwards more between two
device events, and prints one JSON line with the time per forward and a checksum of the prediction.
  python tools/eval_forward_ab.py --model baseline --engine s3 --rounds 3 \\
      --arm P:fused=0,CAD_LIB=libcad_hip_parent.so --arm U:fused=0 --arm F:fused=1
Prints one JSON line per run and a summary: per arm the median, the spread (max - min over its runs), the ratio to
the first arm, and whether its checksum equals the first arm's.  Every child runs under --timeout seconds; the first
failing child ends the script."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = {"f32": 0, "s3": 1, "bf16": 2}
MODELS = {"baseline": "BaselineUNet", "film": "IntrinsicsConditionedUNet", "rayfilm": "RayConditionedUNet"}

ap = argparse.ArgumentParser()
ap.add_argument("--arm", action="append", default=[], help="NAME:fused=0|1[,VAR=value...]; repeat per arm")
ap.add_argument("--model", choices=list(MODELS), default="baseline")
ap.add_argument("--engine", choices=list(ENGINES), default="s3")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--forwards", type=int, default=20)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--features", type=int, default=64)
ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)   # fused=0|1: time one arm in this process
args = ap.parse_args()


def child(fused):
    import torch
    sys.path.insert(0, ROOT)
    import cad_pkg
    cad = cad_pkg.load()
    from cad_amd import synthetic
    from oracle import cad_oracle as O
    lib = cad.load_library()
    assert lib.cad_set_gemm_engine(ENGINES[args.engine]) == 0
    dev = torch.device("cuda", 0)
    f, B, H, W = args.features, args.batch, args.height, args.width
    shape = (3, f, 10.0) if args.model == "baseline" else (3, f, 4, 10.0)
    m = getattr(cad, MODELS[args.model])(*shape, batch=B, height=H, width=W)
    state = dict(O.init_params(f, seed=3, model=args.model))   # the same weights in every arm
    state.update(O.init_buffers(f, model=args.model))
    m.load_state_dict(state)
    m.eval()
    if fused:
        m.fused_eval(True)   # (an older variant build has no such entry: that arm cannot be a fused one)
    rgb, _, K = synthetic.device_batch(B, H, W, dev)
    cam = cad.camera_from_K(K) if m.conditioned else None
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)

    def fwd():
        return m.forward_cam(rgb, cam, out=out) if m.conditioned else m.forward(rgb, out=out)
    for _ in range(args.warmup):
        fwd()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(args.forwards):
        fwd()
    t1.record()
    torch.cuda.synchronize()
    convs = list(m.fused_eval_convs()) if hasattr(lib, "cad_unet_fused_eval_convs") else None
    print(json.dumps({"ms_per_forward": t0.elapsed_time(t1) / args.forwards, "fused_convs": convs,
                      "checksum": hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]}), flush=True)


if args.child is not None:
    child(args.child == "fused=1")
    sys.exit(0)

arms = []
for spec in args.arm:
    name, _, rest = spec.partition(":")
    kv = dict(x.split("=", 1) for x in filter(None, rest.split(",")))
    fused = kv.pop("fused", "0")
    if not name or fused not in ("0", "1"):
        sys.exit(f"--arm '{spec}': expected NAME:fused=0|1[,VAR=value...]")
    arms.append((name, fused, kv))
if len(arms) < 2:
    sys.exit("give at least two --arm")
passthrough = []
for k in ("model", "engine", "warmup", "forwards", "batch", "height", "width", "features"):
    passthrough += ["--" + k, str(getattr(args, k))]
res = {name: [] for name, _, _ in arms}
for rnd in range(args.rounds):
    order = arms[rnd % len(arms):] + arms[:rnd % len(arms)]   # every arm takes every position in turn
    for name, fused, kv in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "fused=" + fused, *passthrough]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **kv), timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"arm": name, "round": rnd, "error": f"no result within {args.timeout} s"}), flush=True)
            sys.exit(1)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            print(json.dumps({"arm": name, "round": rnd, "returncode": r.returncode, "error": r.stderr[-2000:]}), flush=True)
            sys.exit(1)
        out = dict(json.loads(lines[-1]), arm=name, round=rnd, fused=int(fused), env=kv, model=args.model, engine=args.engine)
        res[name].append(out)
        print(json.dumps(out), flush=True)
first = arms[0][0]
base = statistics.median(x["ms_per_forward"] for x in res[first])
summary = {"summary": True, "model": args.model, "engine": args.engine, "shape": [args.batch, args.height, args.width],
           "features": args.features, "forwards": args.forwards, "rounds": args.rounds, "arms": {}}
for name, _, _ in arms:
    ms = [x["ms_per_forward"] for x in res[name]]
    med = statistics.median(ms)
    summary["arms"][name] = {"median_ms": round(med, 3), "spread_ms": round(max(ms) - min(ms), 3),
                             "over_" + first: round(med / base, 4), "fused_convs": res[name][-1]["fused_convs"],
                             "checksum": res[name][-1]["checksum"],
                             "same_output_as_" + first: all(x["checksum"] == res[first][0]["checksum"] for x in res[name])}
print(json.dumps(summary), flush=True)
