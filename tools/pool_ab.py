#!/usr/bin/env python3
"""Statistics pooling (pool_stats_kernel) against the default time-mean at the bench shape: WavLM-base bf16,
256 clips of 3 s, layers [12, 11, 10, 6].

  per launch   pool_stats launches inside the forward (sse_profile_read tags "pool_stats:*") for mean_std,
               mean_std_max and mean_std over windows (50, 25); and the kernel on its own (sse_pool) on a
               [256, 149, 768] bf16 tensor, every variant plus the plain mean routed through the same kernel.
               pool_mean_kernel carries no profile tag: the two kernels are compared in one process from a
               kernel trace of `--trace-phases N` (each variant's embed N times, default first), reduced with
               `--reduce-trace kt_kernel_trace.csv`: pool_mean launches are the default phase, the pool_stats
               launches in start order are the three variants' phases, equal in number.
  clips/s      embed(pool=...) against the default embed(), interleaved over --rounds rounds.

Usage: python tools/pool_ab.py [--out profiles/pool_stats_ab.json] [--rounds 3] [--steps 5] [--batch 256]
       rocprofv3 --kernel-trace -d DIR -o kt --output-format csv -- python tools/pool_ab.py --trace-phases 10
       python tools/pool_ab.py --reduce-trace DIR/.../kt_kernel_trace.csv [--merge profiles/pool_stats_ab.json]"""
import argparse
import csv
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

importlib.import_module("stuttering-speech-representation_amd")
from ssr_amd import config as C, synth  # noqa: E402
from ssr_amd.model import SSEModel, pool_states  # noqa: E402

VARIANTS = {"default": {}, "mean_std": dict(pool="mean_std"), "mean_std_max": dict(pool="mean_std_max"),
            "mean_std_w50h25": dict(pool="mean_std", window=50, hop=25)}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def reduce_trace(path, merge):
    """Kernel-trace rows of a --trace-phases run -> us per launch of pool_mean_kernel and of each pool_stats phase."""
    with open(path, newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "pool_mean_kernel" in r["Kernel_Name"] or "pool_stats_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda rs: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rs]   # noqa: E731
    med = lambda v: sorted(v)[len(v) // 2] if v else None   # noqa: E731

    def stat(v):
        # the half-batches of a split call run on two streams: a pooling launch either has the CUs to itself or
        # shares them with the other half's GEMM; the two modes are reported apart (split at 30 us)
        alone, shared = [x for x in v if x < 30.0], [x for x in v if x >= 30.0]
        return {"launches": len(v), "mean": sum(v) / len(v), "median": med(v), "min": min(v), "max": max(v),
                "alone": {"launches": len(alone), "median": med(alone)},
                "shared": {"launches": len(shared), "median": med(shared)}}
    mean = dur([r for r in rows if "pool_mean_kernel" in r["Kernel_Name"]])
    st = [r for r in rows if "pool_stats_kernel" in r["Kernel_Name"]]
    names = [k for k in VARIANTS if k != "default"]
    assert mean and st and len(st) % len(names) == 0, (len(mean), len(st))
    n = len(st) // len(names)
    out = {"pool_mean_kernel": stat(mean)}
    for i, k in enumerate(names):
        out["pool_stats_kernel:" + k] = stat(dur(st[i * n:(i + 1) * n]))
    base = out["pool_mean_kernel"]
    for k, v in out.items():
        v["vs_pool_mean"] = {"mean": v["mean"] / base["mean"],
                             "alone": v["alone"]["median"] / base["alone"]["median"] if v["alone"]["median"] and base["alone"]["median"] else None,
                             "shared": v["shared"]["median"] / base["shared"]["median"] if v["shared"]["median"] and base["shared"]["median"] else None}
    print(json.dumps(out))
    if merge:
        with open(merge) as fh:
            res = json.load(fh)
        res["kernel_trace_us"] = out
        with open(merge, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-phases", type=int, default=0, metavar="N",
                    help="only run each variant's embed N times, in order (for a kernel trace)")
    ap.add_argument("--reduce-trace", default=None, metavar="CSV")
    ap.add_argument("--merge", default=None, metavar="JSON", help="--reduce-trace: add the result to this file")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    if a.reduce_trace:
        return reduce_trace(a.reduce_trace, a.merge)
    B, L, idx = a.batch, 48000, [12, 11, 10, 6]
    m = SSEModel(C.WAVLM_BASE, synth.synth_wavlm_state_dict(C.WAVLM_BASE, seed=7), device="cuda:0", dtype="bf16")
    wave = torch.from_numpy(synth.synth_clips(B, L, seed=1234)).cuda()
    calls = {k: (lambda kw=kw: m.embed(wave, idx, **kw)) for k, kw in VARIANTS.items()}
    # warm-up: workspace, streams (a trace run warms the default only, so that the pool_stats launches of the trace
    # are the three phases and nothing else; medians are reported)
    for f in ([calls["default"]] if a.trace_phases else calls.values()):
        f()
        f()
    torch.cuda.synchronize()
    if a.trace_phases:
        for f in calls.values():
            for _ in range(a.trace_phases):
                f()
            torch.cuda.synchronize()
        return
    res = {"shape": {"model": "wavlm-base", "dtype": "bf16", "B": B, "L": L, "layers": idx}, "in_model_us": {},
           "hook_us": {}, "clips_per_s": {}}
    for k, f in calls.items():
        if k == "default":
            continue
        m.profile_start()
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        us = [1e3 * ms for tag, ms, _, _ in m.profile_read() if tag.startswith("pool_stats")]
        m.profile_stop()
        res["in_model_us"][k] = {"launches": len(us), "mean": sum(us) / max(len(us), 1), "min": min(us), "max": max(us)}
    x = (torch.randn((B, 149, 768), device="cuda") + 100.0).bfloat16()
    hooks = dict(VARIANTS, mean_via_pool_stats=dict(pool="mean"), max=dict(pool="max"))
    del hooks["default"]
    for k, kw in hooks.items():
        f = lambda kw=kw: pool_states(x, **kw)   # noqa: E731
        timed(f, 5)
        res["hook_us"][k] = 1e3 * min(timed(f, 20) for _ in range(3))
    per = {k: [] for k in calls}
    for _ in range(a.rounds):
        for k, f in calls.items():
            per[k].append(B / (1e-3 * timed(f, a.steps)))
    res["clips_per_s"] = {k: {"rounds": v, "median": sorted(v)[len(v) // 2]} for k, v in per.items()}
    base = res["clips_per_s"]["default"]["median"]
    for k, v in res["clips_per_s"].items():
        v["vs_default"] = v["median"] / base
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
