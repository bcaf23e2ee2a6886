"""Per-kernel table of the S3 window convolutions from two rocprofv3 passes of one build:

  python profiles/win_compare.py <trace dir> <pmc dir> [<trace dir B> <pmc dir B>] > table.md

trace dir: rocprofv3 --kernel-trace --stats output; pmc dir: one --pmc pass with SQ_INSTS_VALU,
SQ_VALU_MFMA_BUSY_CYCLES, SQ_WAVE_CYCLES, SQ_WAIT_ANY, SQ_WAIT_INST_ANY, SQ_ACTIVE_INST_ANY, GRBM_GUI_ACTIVE
(the passes are separate runs of the same command; CAD_SIDE_WGRAD=0 so every GEMM runs alone).  Columns as
in profiles/summarize.py: clock = GRBM_GUI_ACTIVE / 8 XCDs / average duration, MFMA busy =
SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8), stalled = SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES;
VALU = SQ_INSTS_VALU per launch (wave instructions, summed over the chip).  With two builds the rows are
matched by kernel name less the weight-twin template flag (", true") and the ratios B / A are added.
"""
import sys

from summarize import durations, pmc

NAMES = ["SQ_INSTS_VALU", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY", "GRBM_GUI_ACTIVE"]


def table(trace, pm):
    dur = durations(trace)
    c = {n: pmc(pm, n) for n in NAMES}
    rows = {}
    for k, v in dur.items():
        if "k_conv3x3_win_s3" not in k:
            continue
        avg = {n: (sum(c[n][k]) / len(c[n][k]) if c[n].get(k) else 0.0) for n in NAMES}
        ns = sum(v) / len(v)
        act = avg["GRBM_GUI_ACTIVE"] / 8
        rows[k.replace(" >", ">").replace(", true>", ">")] = {
            "launches": len(v), "us": ns / 1e3, "valu": avg["SQ_INSTS_VALU"], "ghz": act / ns if ns else 0.0,
            "mfma": avg["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024 * act) if act else 0.0,
            "stalled": avg["SQ_WAIT_INST_ANY"] / avg["SQ_WAVE_CYCLES"] if avg["SQ_WAVE_CYCLES"] else 0.0}
    return rows


def main():
    a = table(sys.argv[1], sys.argv[2])
    b = table(sys.argv[3], sys.argv[4]) if len(sys.argv) > 4 else None
    f = "{us:.1f} | {valu:.3e} | {mfma:.3f} | {stalled:.2f} | {ghz:.2f}"
    head = "avg us | VALU / launch | MFMA busy | stalled | GHz"
    if b is None:
        print(f"| kernel | launches | {head} |\n|---|---|---|---|---|---|---|")
        for k, r in sorted(a.items(), key=lambda kv: -kv[1]["us"] * kv[1]["launches"]):
            print(f"| `{k}` | {r['launches']} | " + f.format(**r) + " |")
        return
    print(f"| kernel | launches | A: {head} | B: {head} | us B/A | VALU B/A |")
    print("|---|---|" + "---|" * 12)
    ta = tb = 0.0
    for k, r in sorted(a.items(), key=lambda kv: -kv[1]["us"] * kv[1]["launches"]):
        s = b.get(k)
        if not s:
            continue
        ta += r["us"] * r["launches"]
        tb += s["us"] * s["launches"]
        print(f"| `{k}` | {r['launches']} | " + f.format(**r) + " | " + f.format(**s) +
              f" | {s['us'] / r['us']:.3f} | {s['valu'] / r['valu'] if r['valu'] else 0:.3f} |")
    print(f"\nsum over the launches of the traced run: A {ta / 1e3:.2f} ms, B {tb / 1e3:.2f} ms ({tb / ta:.4f})")


if __name__ == "__main__":
    main()
