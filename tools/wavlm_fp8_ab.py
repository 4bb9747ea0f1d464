#!/usr/bin/env python3
"""WavLM-large: the MX-fp8 encoder (dtype="fp8") against the bf16 path, same tree, same box, one process.

Both models embed the bench workload (256 clips of 3 s, layers [24, 23, 22, 12], do_normalize) interleaved over
--rounds rounds; reported are ms per step and clips/s per round and their medians, the fp8 / bf16 ratio, the
fp8 - bf16 rel-L2 / cosine of the embeddings, and for each model the per-launch profile (sse_profile_read) summed by
tag -- the conv front end, the positional conv, the attention and the out-projection are the same bf16 kernels in
both, so the tags name where a gain comes from and what bounds it.

Usage: python tools/wavlm_fp8_ab.py [--out profiles/wavlm_fp8_ab.json] [--rounds 3] [--steps 5] [--batch 256]"""
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

L = 48000
DTYPES = ("bf16", "fp8")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def by_tag(m, fn):
    """One profiled call -> {tag: launches, ms, TFLOP/s} in launch order of first appearance, and the total ms."""
    m.profile_start()
    fn()
    torch.cuda.synchronize()
    rows = m.profile_read()
    m.profile_stop()
    out = {}
    for tag, ms, fl, _ in rows:
        n, t, f = out.get(tag, (0, 0.0, 0.0))
        out[tag] = (n + 1, t + ms, f + fl)
    return ({k: {"launches": n, "ms": t, "tflops": f / (1e9 * t) if t > 0 and f > 0 else None}
             for k, (n, t, f) in out.items()}, sum(t for _, t, _ in out.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3 (the comparison is a median over interleaved rounds)")
    spec, B = C.WAVLM_LARGE, a.batch
    idx = spec.default_layer_indices()
    sd = synth.synth_wavlm_state_dict(spec, seed=9)
    models = {d: SSEModel(spec, sd, device="cuda:0", dtype=d, do_normalize=True) for d in DTYPES}
    wave = torch.from_numpy(synth.synth_clips(B, L, seed=1234)).cuda()
    outs = {d: torch.empty((B, len(idx), spec.hidden), device="cuda:0") for d in DTYPES}
    bufs = {d: torch.empty(m.workspace_bytes(B, L), dtype=torch.uint8, device="cuda:0") for d, m in models.items()}
    calls = {d: (lambda d=d: models[d].embed(wave, idx, out=outs[d], workspace=bufs[d])) for d in DTYPES}
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    ms = {d: [] for d in DTYPES}
    for _ in range(a.rounds):
        for d, f in calls.items():
            ms[d].append(timed(f, a.steps))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "model": spec.name, "B": B, "clip_samples": L, "layers_pooled": idx,
           "rounds": a.rounds, "steps": a.steps}
    for d in DTYPES:
        prof, total = by_tag(models[d], calls[d])
        res[d] = {"workspace_bytes": bufs[d].numel(), "ms_per_step": {"rounds": ms[d], "median": med(ms[d])},
                  "clips_per_s": {"rounds": [B / (1e-3 * t) for t in ms[d]], "median": B / (1e-3 * med(ms[d]))},
                  "profile_ms_by_tag": prof, "profile_ms_total": total}
    res["fp8_vs_bf16"] = {"ms_per_step": res["fp8"]["ms_per_step"]["median"] / res["bf16"]["ms_per_step"]["median"],
                          "clips_per_s": res["fp8"]["clips_per_s"]["median"] / res["bf16"]["clips_per_s"]["median"]}
    x, y = outs["fp8"].double(), outs["bf16"].double()
    res["fp8_minus_bf16"] = {"rel_l2_max": float(((x - y).norm(dim=-1) / y.norm(dim=-1)).max()),
                             "cos_min": float(torch.nn.functional.cosine_similarity(x, y, dim=-1).min())}
    print(json.dumps({k: res[k] for k in ("model", "B", "fp8_vs_bf16", "fp8_minus_bf16")}), flush=True)
    for d in DTYPES:
        print(d, f"{res[d]['ms_per_step']['median']:.2f} ms/step, {res[d]['clips_per_s']['median']:.0f} clips/s;",
              ", ".join(f"{t} {v['ms']:.2f}" for t, v in res[d]["profile_ms_by_tag"].items()), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
