#!/usr/bin/env python3
"""wav2vec 2.0 / HuBERT base: the bias-free spec (num_buckets=0) against the route a user could fake before it --
a WavLM-base-kind model with a zero relative-position table and dummy gate weights.  Same weights, same tree, same
box, one process.

Both models embed the bench workload (bf16, 256 clips of 3 s, layers [12, 11, 10, 6]) interleaved over --rounds
rounds.  Reported: ms per step and clips/s of every round and their medians for (a) the old route and (b) the
bias-free spec, the round-to-round spread of each (max - min over its identical rounds, relative to the median),
the b / a ratio, whether (b) is slower than (a) by more than that spread, the b - a rel-L2 of the embeddings, and
the per-launch profile (sse_profile_read) summed by tag -- gemm:qkv (2304 instead of 2560 columns) and attn (no
gate sigmoids, no bias add) are where the two differ.

Usage: python tools/w2v_ab.py [--out profiles/w2v_ab.json] [--rounds 5] [--steps 10] [--batch 256]"""
import argparse
import dataclasses
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

importlib.import_module("stuttering-speech-representation_amd")
from ssr_amd import config as C, synth  # noqa: E402
from ssr_amd.model import SSEModel  # noqa: E402

L = 48000
ROUTES = ("old_zero_bias", "bias_free")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def by_tag(m, fn):
    m.profile_start()
    fn()
    torch.cuda.synchronize()
    rows = m.profile_read()
    m.profile_stop()
    out = {}
    for tag, ms, _, _ in rows:
        n, t = out.get(tag, (0, 0.0))
        out[tag] = (n + 1, t + ms)
    return {k: {"launches": n, "ms": t} for k, (n, t) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3 (the spread is taken over identical interleaved rounds)")
    B = a.batch
    free = C.WAV2VEC2_BASE
    sd = synth.synth_wavlm_state_dict(free, seed=13)
    old = dataclasses.replace(free, num_buckets=320, max_distance=800, name="wavlm-base-kind+zero-bias")
    gates = synth.synth_wavlm_state_dict(old, seed=5)
    sd_old = dict(sd)
    for k, v in gates.items():
        if k.endswith("rel_attn_embed.weight"):
            sd_old[k] = np.zeros_like(v)
        elif "gru_rel_pos" in k:
            sd_old[k] = v
    specs = {"old_zero_bias": (old, sd_old), "bias_free": (free, sd)}
    models = {r: SSEModel(s, w, device="cuda:0", dtype=a.dtype) for r, (s, w) in specs.items()}
    idx = free.default_layer_indices()
    wave = torch.from_numpy(synth.synth_clips(B, L, seed=1234)).cuda()
    outs = {r: torch.empty((B, len(idx), free.hidden), device="cuda:0") for r in ROUTES}
    bufs = {r: torch.empty(m.workspace_bytes(B, L), dtype=torch.uint8, device="cuda:0") for r, m in models.items()}
    calls = {r: (lambda r=r: models[r].embed(wave, idx, out=outs[r], workspace=bufs[r])) for r in ROUTES}
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    ms = {r: [] for r in ROUTES}
    for _ in range(a.rounds):
        for r, f in calls.items():
            ms[r].append(timed(f, a.steps))
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "shape": "768/12/12/3072 (wav2vec2-base, hubert-base)", "dtype": a.dtype,
           "B": B, "clip_samples": L, "layers_pooled": idx, "rounds": a.rounds, "steps": a.steps}
    for r in ROUTES:
        m = med(ms[r])
        res[r] = {"spec": specs[r][0].name, "workspace_bytes": bufs[r].numel(),
                  "ms_per_step": {"rounds": ms[r], "median": m},
                  "clips_per_s": {"rounds": [B / (1e-3 * t) for t in ms[r]], "median": B / (1e-3 * m)},
                  "round_spread_rel": (max(ms[r]) - min(ms[r])) / m, "profile_ms_by_tag": by_tag(models[r], calls[r])}
    ratio = res["bias_free"]["ms_per_step"]["median"] / res["old_zero_bias"]["ms_per_step"]["median"]
    spread = max(res[r]["round_spread_rel"] for r in ROUTES)
    x, y = outs["bias_free"].double(), outs["old_zero_bias"].double()
    res["bias_free_vs_old"] = {"ms_per_step_ratio": ratio, "clips_per_s_ratio": 1.0 / ratio,
                               "round_spread_rel": spread, "not_slower_beyond_spread": bool(ratio <= 1.0 + spread),
                               "rel_l2_max": float(((x - y).norm(dim=-1) / y.norm(dim=-1)).max())}
    print(json.dumps(res["bias_free_vs_old"]), flush=True)
    for r in ROUTES:
        print(r, f"{res[r]['ms_per_step']['median']:.2f} ms/step, {res[r]['clips_per_s']['median']:.0f} clips/s, "
              f"spread {100 * res[r]['round_spread_rel']:.2f} %;",
              ", ".join(f"{t} {v['ms']:.2f}" for t, v in res[r]["profile_ms_by_tag"].items()), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 0 if res["bias_free_vs_old"]["not_slower_beyond_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
