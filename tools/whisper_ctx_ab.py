#!/usr/bin/env python3
"""Whisper audio context (SSEModel.embed(frames=F)) at equal GEMM rows, on 3 s clips.

Two configurations per (model, dtype), interleaved over --rounds rounds on one box:

  full   B0 clips, no context: the reference's 1500 encoder frames (30 s pad) per clip; B0 = the bench batch
         (bench.py: 64 for bf16, 128 for fp8)
  ctx    10 B0 clips, frames=150: the 150 frames that cover a 3 s clip

Both steps run B * F = 1500 B0 GEMM rows; ctx has a tenth of the attention FLOPs (B F^2) and a tenth of the log-mel
frames per clip, so its step must not be slower than full's beyond the box spread; its clips/s is then ~10x.
Reported: ms per step and clips/s per round and their medians, the step-time and clips/s ratios, and for each
configuration the per-launch profile (sse_profile_read) summed by tag, which names the kernel if ctx's step is
the slower one.

Usage: python tools/whisper_ctx_ab.py [--out profiles/whisper_ctx_ab.json] [--rounds 3] [--steps 3]
                                      [--models whisper-small,whisper-large-v2] [--dtypes bf16,fp8]"""
import argparse
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

importlib.import_module("stuttering-speech-representation_amd")
from ssr_amd import config as C, synth  # noqa: E402
from ssr_amd.model import SSEModel  # noqa: E402

SPECS = {"whisper-small": C.WHISPER_SMALL, "whisper-large-v2": C.WHISPER_LARGE_V2}
BENCH_BATCH = {"bf16": 64, "fp8": 128}
L, F_CTX = 48000, 150


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def by_tag(m, fn):
    """One profiled call -> {tag: [launches, ms]} in launch order of first appearance, and the total."""
    m.profile_start()
    fn()
    torch.cuda.synchronize()
    rows = m.profile_read()
    m.profile_stop()
    out = {}
    for tag, ms, _, _ in rows:
        n, t = out.get(tag, (0, 0.0))
        out[tag] = (n + 1, t + ms)
    return {k: {"launches": n, "ms": t} for k, (n, t) in out.items()}, sum(t for _, t in out.values())


def run(name, dtype, rounds, steps):
    spec = SPECS[name]
    m = SSEModel(spec, synth.synth_whisper_state_dict(spec, seed=11), device="cuda:0", dtype=dtype)
    idx = spec.default_layer_indices()
    B0 = BENCH_BATCH[dtype]
    cfgs = {"full": (B0, None), "ctx": (10 * B0, F_CTX)}
    waves = {k: torch.from_numpy(synth.synth_clips(B, L, seed=1234)).cuda() for k, (B, _) in cfgs.items()}
    ws = {k: m.workspace_bytes(B, L, frames=F) for k, (B, F) in cfgs.items()}
    buf = torch.empty(max(ws.values()), dtype=torch.uint8, device="cuda:0")
    outs = {k: torch.empty((B, len(idx), spec.hidden), device="cuda:0") for k, (B, _) in cfgs.items()}
    calls = {k: (lambda k=k, F=F: m.embed(waves[k], idx, out=outs[k], workspace=buf, frames=F))
             for k, (_, F) in cfgs.items()}
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            ms[k].append(timed(f, steps))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"model": name, "dtype": dtype, "clip_samples": L, "layers_pooled": idx, "rounds": rounds, "steps": steps}
    for k, (B, F) in cfgs.items():
        prof, total = by_tag(m, calls[k])
        res[k] = {"B": B, "frames": F or spec.max_positions, "gemm_rows": B * (F or spec.max_positions),
                  "workspace_bytes": ws[k], "ms_per_step": {"rounds": ms[k], "median": med(ms[k])},
                  "clips_per_s": {"rounds": [B / (1e-3 * t) for t in ms[k]], "median": B / (1e-3 * med(ms[k]))},
                  "profile_ms_by_tag": prof, "profile_ms_total": total}
    res["ctx_vs_full"] = {"ms_per_step": res["ctx"]["ms_per_step"]["median"] / res["full"]["ms_per_step"]["median"],
                          "clips_per_s": res["ctx"]["clips_per_s"]["median"] / res["full"]["clips_per_s"]["median"]}
    # the tags whose summed time grew the most from full to ctx (equal rows: a GEMM tag should not grow)
    grow = {t: res["ctx"]["profile_ms_by_tag"][t]["ms"] - res["full"]["profile_ms_by_tag"].get(t, {"ms": 0.0})["ms"]
            for t in res["ctx"]["profile_ms_by_tag"]}
    res["ctx_minus_full_ms_by_tag"] = dict(sorted(grow.items(), key=lambda kv: -kv[1]))
    del m
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--models", default="whisper-small,whisper-large-v2")
    ap.add_argument("--dtypes", default="bf16,fp8")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3 (the comparison is a median over interleaved rounds)")
    res = {"device": torch.cuda.get_device_name(0), "runs": []}
    for name in a.models.split(","):
        for dtype in a.dtypes.split(","):
            r = run(name, dtype, a.rounds, a.steps)
            print(json.dumps({k: r[k] for k in ("model", "dtype", "ctx_vs_full")}), flush=True)
            res["runs"].append(r)
            if a.out:   # written after every run: a long job leaves what it finished
                with open(a.out, "w") as fh:
                    json.dump(res, fh, indent=1)
                    fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
