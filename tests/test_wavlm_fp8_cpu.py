"""The evidence behind dtype="fp8" for WavLM (CPU): tools/wavlm_mx_emulate.py runs the reference's arithmetic with the
QKV / fc1 / fc2 operands in MX-fp8 (bf16 elsewhere) against the reference-run fixtures.  The stable-LN model
(WavLM-large) holds the project's fp8 bar, 0.08 rel-L2 / 0.995 cosine, on the format alone; the post-LN model
(WavLM-base) does not -- which is why sse_model_create refuses it."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

MX8 = "qkv + ffn1 + ffn2 mx8"


def _emulate(fixture, name, n):
    import wavlm_mx_emulate as W
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    r = W.emulate(fixture, W.ASSIGNMENTS[name], n)
    print(fixture, name, r["rel_l2_max"], r["cos_min"])
    return r


def test_stable_ln_wavlm_holds_the_fp8_bar_on_format_alone():
    bf = _emulate("wavlm_large", "all bf16", 1)
    mx = _emulate("wavlm_large", MX8, 1)
    assert mx["rel_l2_max"] <= 0.08 and mx["cos_min"] >= 0.995
    assert mx["rel_l2_max"] > bf["rel_l2_max"] and mx["cos_min"] < bf["cos_min"]


def test_post_ln_wavlm_misses_the_fp8_bar_on_format_alone():
    assert _emulate("wavlm_base", MX8, 2)["rel_l2_max"] > 0.08
