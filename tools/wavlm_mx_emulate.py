#!/usr/bin/env python3
"""Format-forced error of MX-fp8 encoder GEMMs in WavLM (CPU; the evidence behind dtype="fp8" for stable-LN WavLM).

oracle/emulate.py's ``_Patch`` runs the reference's ATen call sequence with the GEMM operands of chosen stages
rounded to an operand format.  This wrapper adds the format "mx8": activations rounded to bf16 (the residual
stream's and the LayerNorm input's type), then quantised to MX-fp8 along K in blocks of 32 (``oracle.emulate._mx8``);
the weights quantised likewise.  The assignment of the GPU path puts the qkv (q / k / v and gru_rel_pos_linear),
ffn1 and ffn2 stages in mx8 and conv / proj / oproj / attn in bf16 -- an ideal kernel in those formats, independent
of any HIP code, against the reference-run fixtures.

Usage: python tools/wavlm_mx_emulate.py [--out profiles/wavlm_fp8_emulated.json] [--threads 16]"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

importlib.import_module("stuttering-speech-representation_amd")
from oracle import emulate as E  # noqa: E402
from ssr_amd import config as C, synth  # noqa: E402

BF16 = {st: "bf16" for st in ("conv", "proj", "qkv", "attn", "oproj", "ffn1", "ffn2")}
ASSIGNMENTS = {
    "all bf16": BF16,
    "qkv + ffn1 + ffn2 mx8": {**BF16, "qkv": "mx8", "ffn1": "mx8", "ffn2": "mx8"},
    "plus oproj mx8": {**BF16, "qkv": "mx8", "ffn1": "mx8", "ffn2": "mx8", "oproj": "mx8"},
    "ffn1 + ffn2 only": {**BF16, "ffn1": "mx8", "ffn2": "mx8"},
    "qkv only": {**BF16, "qkv": "mx8"},
}
# fixture -> (spec, weight seed, clip seed, clips drawn, do_normalize, reference key): tests/golden/make_golden.py
FIXTURES = {"wavlm_large": (C.WAVLM_LARGE, 9, 77, 3, True, "emb"),
            "wavlm_base": (C.WAVLM_BASE, 7, 1234, 16, False, "emb_norm0")}
_ATEN = {}


def _product(fn, x, w, fmt):
    if fmt == "mx8":
        return fn(E._mx8(x.bfloat16().float(), -1), E._mx8(w, -1))
    return _PRODUCT(fn, x, w, fmt)


_PRODUCT = E.emulated_product


def emulate(fixture: str, assignment: dict, n_clips: int) -> dict:
    """Max rel-L2 / min cosine of the first n_clips of the fixture under a stage -> format assignment."""
    spec, wseed, cseed, drawn, norm, key = FIXTURES[fixture]
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{fixture}.npz"))
    idx = [int(i) for i in g["layer_indices"]]
    if fixture not in _ATEN:   # weight synthesis dominates: once per fixture
        o = E.WavLMAten(spec, synth.synth_wavlm_state_dict(spec, seed=wseed))
        _ATEN[fixture] = (o, {id(v): E.stage_of(k) for k, v in o.w.items() if E.stage_of(k)})
    o, ids = _ATEN[fixture]
    clips = synth.synth_clips(drawn, 48000, seed=cseed)[:n_clips]
    E.emulated_product = _product
    try:
        with torch.no_grad(), E._Patch(assignment, ids):
            got = o.embed(clips, idx, norm)
    finally:
        E.emulated_product = _PRODUCT
    rel, cos = E._rel_cos(got, g[key][:n_clips])
    return {"rel_l2_max": float(rel.max()), "cos_min": float(cos.min()), "clips": n_clips, "layers": idx}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    torch.set_num_threads(a.threads)
    rows = [("wavlm_large", "all bf16", 3), ("wavlm_large", "qkv + ffn1 + ffn2 mx8", 3),
            ("wavlm_large", "plus oproj mx8", 1), ("wavlm_base", "all bf16", 4),
            ("wavlm_base", "qkv + ffn1 + ffn2 mx8", 4), ("wavlm_base", "ffn1 + ffn2 only", 4),
            ("wavlm_base", "qkv only", 4)]
    res = {"format": "mx8 = MX-fp8 (e4m3, E8M0 scale per 32 along K) of bf16(x) and of w; other stages bf16",
           "bar": {"rel_l2_max": 0.08, "cos_min": 0.995}, "rows": []}
    print(f"{'fixture':12s} {'assignment':24s} clips  max rel-L2  min cosine")
    for fixture, name, n in rows:
        r = {"fixture": fixture, "assignment": name, **emulate(fixture, ASSIGNMENTS[name], n)}
        res["rows"].append(r)
        print(f"{fixture:12s} {name:24s} {n:5d}  {r['rel_l2_max']:.4f}      {r['cos_min']:.5f}", flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
