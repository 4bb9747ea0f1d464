"""Shared inputs of the wav2vec 2.0 / HuBERT tests (test_w2v_cpu.py, test_gpu_w2v.py): the fixtures of
tests/golden/make_golden_w2v.py, their weights and clips rebuilt from the manifest's seeds, and the OLD route to
the same function -- a WavLM-kind spec whose relative-position table is zero (the gate multiplies it, so any gate
tensors give the bias-free network)."""
import dataclasses
import functools
import json
import os

import numpy as np

from conftest import GOLDEN
from ssr_amd import config as C, synth

W2V_SPEC = C.WAV2VEC2_BASE
HUB_SPEC = dataclasses.replace(C.HUBERT_LARGE, layers=4, name="hubert-large4")


@functools.lru_cache(maxsize=None)
def manifest():
    with open(os.path.join(GOLDEN, "manifest_w2v.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def golden(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz")))


@functools.lru_cache(maxsize=None)
def weights(name):
    spec = {"wav2vec2_base": W2V_SPEC, "hubert_large4": HUB_SPEC}[name]
    return synth.synth_wavlm_state_dict(spec, seed=manifest()[name]["weight_seed"])


@functools.lru_cache(maxsize=None)
def clips(name, which):
    """The clips of one fixture entry (manifest "clips": which -> [count, samples, first_clip])."""
    m = manifest()[name]
    n, samples, first = m["clips"][which]
    return synth.synth_clips(n, samples, seed=m["clip_seed"], first_clip=first)


def old_route(spec, sd, gate_seed=5):
    """(WavLM-kind spec, state dict) computing the same function as the bias-free (spec, sd): the default
    320-bucket table, all zeros, and random gate tensors (the gate only ever scales the table)."""
    old = dataclasses.replace(spec, num_buckets=320, max_distance=800, name=spec.name + "+zero-bias")
    ref = synth.synth_wavlm_state_dict(old, seed=gate_seed)
    out = dict(sd)
    for k, v in ref.items():
        if k.endswith("rel_attn_embed.weight"):
            out[k] = np.zeros_like(v)
        elif "gru_rel_pos" in k:
            out[k] = v
    assert set(out) == set(ref)
    return old, out
