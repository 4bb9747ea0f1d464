"""wav2vec 2.0 / HuBERT on the bias-free path, host side (no GPU): the config -> spec mapping and its refusals,
the canonical weight order with ``num_buckets=0``, and the claim the design rests on -- a wav2vec 2.0 / HuBERT
encoder is a WavLM encoder whose relative-position table is zero -- pinned by the unchanged numpy oracle
against fixtures the reference's own glue produced from transformers' Wav2Vec2Model / HubertModel
(tests/golden/make_golden_w2v.py)."""
import ctypes
import dataclasses
import hashlib

import numpy as np
import pytest

import w2v_fixtures as wf
from ssr_amd import config as C, hf

ORACLE_TOL = 1e-5     # tests/test_oracle_golden.py's bar: fp32 restatement vs fp32 reference


def _rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _large_kwargs():
    return dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)


# ---- spec mapping ---------------------------------------------------------------------------------------------
def test_configs_map_to_named_specs():
    from transformers import HubertConfig, Wav2Vec2Config
    assert hf.wav2vec2_spec_from_config(Wav2Vec2Config()) is C.WAV2VEC2_BASE
    assert hf.hubert_spec_from_config(HubertConfig()) is C.HUBERT_BASE
    assert hf.wav2vec2_spec_from_config(Wav2Vec2Config(**_large_kwargs())) is C.WAV2VEC2_LARGE_LV60
    assert hf.hubert_spec_from_config(HubertConfig(**_large_kwargs())) is C.HUBERT_LARGE
    for s in (C.WAV2VEC2_BASE, C.HUBERT_BASE):
        assert (s.hidden, s.layers, s.heads, s.ffn) == (768, 12, 12, 3072)
        assert not s.feat_norm_layer and not s.stable_layer_norm and not s.conv_bias
    for s in (C.WAV2VEC2_LARGE_LV60, C.HUBERT_LARGE):
        assert (s.hidden, s.layers, s.heads, s.ffn) == (1024, 24, 16, 4096)
        assert s.feat_norm_layer and s.stable_layer_norm and s.conv_bias
    for s in (C.WAV2VEC2_BASE, C.HUBERT_BASE, C.WAV2VEC2_LARGE_LV60, C.HUBERT_LARGE):
        assert s.kind == C.KIND_WAVLM and s.num_buckets == 0 and not s.rel_pos_bias
    assert C.WAVLM_BASE.rel_pos_bias and C.WAVLM_LARGE.rel_pos_bias
    # an unnamed shape keeps its fields
    s = hf.hubert_spec_from_config(HubertConfig(num_hidden_layers=4, **{k: v for k, v in _large_kwargs().items()
                                                                        if k != "num_hidden_layers"}))
    assert dataclasses.replace(s, name="") == dataclasses.replace(wf.HUB_SPEC, name="")


@pytest.mark.parametrize("field,kw", [
    ("add_adapter", dict(add_adapter=True)),
    ("conv_pos_batch_norm", dict(conv_pos_batch_norm=True)),
    ("feat_proj_layer_norm", dict(feat_proj_layer_norm=False)),
    ("feat_extract_activation", dict(feat_extract_activation="relu")),
    ("hidden_act", dict(hidden_act="relu")),
    ("feat_extract_norm", dict(feat_extract_norm="batch")),
    ("num_attention_heads", dict(hidden_size=1280, num_attention_heads=16)),      # hubert-xlarge: head width 80
])
def test_refusals_name_the_field(field, kw):
    """Each unsupported field raises NotImplementedError naming it, on the host (no library call is involved:
    the mapping functions never touch libsse.so)."""
    from types import SimpleNamespace
    from transformers import HubertConfig, Wav2Vec2Config
    for fn, cfg in ((hf.wav2vec2_spec_from_config, Wav2Vec2Config), (hf.hubert_spec_from_config, HubertConfig)):
        try:
            c = cfg(**kw)
        except (TypeError, ValueError):     # a config class that validates the field itself: same fields, no checks
            c = SimpleNamespace(**{**cfg().to_dict(), **kw})
        for k, v in kw.items():             # a config class that does not know the field drops it silently
            if getattr(c, k, None) != v:
                c = SimpleNamespace(**{**cfg().to_dict(), **kw})
        with pytest.raises(NotImplementedError, match=field):
            fn(c)


def test_head_width_refused_before_the_library():
    """SSEModel refuses head widths other than 64 with a ValueError before it loads or calls libsse.so (the
    device argument is never reached), and the library's own cfg check agrees."""
    from ssr_amd import _lib
    from ssr_amd.model import SSEModel
    xl = dataclasses.replace(C.HUBERT_LARGE, hidden=1280, heads=16, ffn=5120, layers=2, name="hubert-xlarge-like")
    with pytest.raises(ValueError, match="head width of 64"):
        SSEModel(xl, {}, device="cuda:0")
    assert _lib.lib().sse_weight_floats(ctypes.byref(_lib.make_cfg(xl))) == 0
    neg = _lib.make_cfg(C.WAV2VEC2_BASE)
    neg.num_buckets = -1
    assert _lib.lib().sse_weight_floats(ctypes.byref(neg)) == 0


def test_frames_is_still_the_whisper_context():
    with pytest.raises(ValueError, match="Whisper"):
        C.resolve_frames(C.WAV2VEC2_BASE, 100, 48000)


# ---- canonical weight order -----------------------------------------------------------------------------------
def _numel(specs):
    return sum(int(np.prod(s)) for _, s in specs)


@pytest.mark.parametrize("free,full", [(C.WAV2VEC2_BASE, C.WAVLM_BASE), (C.HUBERT_BASE, C.WAVLM_BASE),
                                       (C.WAV2VEC2_LARGE_LV60, dataclasses.replace(C.WAVLM_LARGE, conv_bias=True)),
                                       (C.HUBERT_LARGE, dataclasses.replace(C.WAVLM_LARGE, conv_bias=True))])
def test_param_specs_drop_exactly_the_bias_tensors(free, full):
    from ssr_amd import _lib
    a, b = C.param_specs(free), C.param_specs(full)
    assert not [k for k, _ in a if "rel_attn_embed" in k or "gru_" in k]
    dropped = [(k, s) for k, s in b if "rel_attn_embed" in k or "gru_" in k]
    assert len(dropped) == 1 + 3 * full.layers
    assert a == [e for e in b if e not in dropped]            # nothing else changes in the order
    assert C.weight_floats(free) == C.weight_floats(full) - _numel(dropped)
    assert _lib.lib().sse_weight_floats(ctypes.byref(_lib.make_cfg(free))) == C.weight_floats(free)
    n_bias = sum(k.startswith("feature_extractor.") and k.endswith(".conv.bias") for k, _ in a)
    assert n_bias == (7 if free.conv_bias else 0)


def test_pack_weights_of_hf_state_dicts():
    """State dicts of transformers' own models (2 layers; with masked_spec_embed, and a ForPreTraining one with
    its quantizer and projection heads under the ``wav2vec2.`` prefix stripped) pack to weight_floats."""
    import torch
    from transformers import HubertConfig, HubertModel, Wav2Vec2Config, Wav2Vec2ForPreTraining, Wav2Vec2Model
    from ssr_amd.model import pack_weights
    torch.manual_seed(0)
    big = {**_large_kwargs(), "num_hidden_layers": 2}
    for cls, cfg, fn in ((Wav2Vec2Model, Wav2Vec2Config(num_hidden_layers=2), hf.wav2vec2_spec_from_config),
                         (HubertModel, HubertConfig(num_hidden_layers=2), hf.hubert_spec_from_config),
                         (Wav2Vec2Model, Wav2Vec2Config(**big), hf.wav2vec2_spec_from_config),
                         (HubertModel, HubertConfig(**big), hf.hubert_spec_from_config)):
        m = cls(cfg)
        spec = fn(m.config)
        sd = m.state_dict()
        assert "masked_spec_embed" in sd
        blob = pack_weights(spec, sd)
        assert blob.size == C.weight_floats(spec) and blob.dtype == np.float32
        if spec.conv_bias:
            assert "feature_extractor.conv_layers.3.conv.bias" in dict(C.param_specs(spec))
    pre = Wav2Vec2ForPreTraining(Wav2Vec2Config(num_hidden_layers=2))
    sd = {k[len("wav2vec2."):] if k.startswith("wav2vec2.") else k: v for k, v in pre.state_dict().items()}
    assert any(k.startswith("quantizer.") for k in sd) and any(k.startswith("project_") for k in sd)
    spec = hf.wav2vec2_spec_from_config(pre.config)
    assert pack_weights(spec, sd).size == C.weight_floats(spec)
    with pytest.raises(KeyError, match="rel_attn_embed"):          # the old failure, on the WavLM mapping
        pack_weights(dataclasses.replace(spec, num_buckets=320), sd)


# the canonical order of the named WavLM specs before this feature (the parent commit's param_specs), written out:
# the keys in order, and the SHA-256 of repr(param_specs(spec)) computed from the parent's config.py
_FRONT_GROUP = ["feature_extractor.conv_layers.0.conv.weight", "feature_extractor.conv_layers.0.layer_norm.weight",
                "feature_extractor.conv_layers.0.layer_norm.bias"] + \
    [f"feature_extractor.conv_layers.{i}.conv.weight" for i in range(1, 7)]
_FRONT_LAYER = [f"feature_extractor.conv_layers.{i}.{n}" for i in range(7)
                for n in ("conv.weight", "layer_norm.weight", "layer_norm.bias")]
_MIDDLE = ["feature_projection.layer_norm.weight", "feature_projection.layer_norm.bias",
           "feature_projection.projection.weight", "feature_projection.projection.bias",
           "encoder.pos_conv_embed.conv.parametrizations.weight.original0",
           "encoder.pos_conv_embed.conv.parametrizations.weight.original1", "encoder.pos_conv_embed.conv.bias",
           "encoder.layer_norm.weight", "encoder.layer_norm.bias", "encoder.layers.0.attention.rel_attn_embed.weight"]
_LAYER = ["attention.q_proj.weight", "attention.q_proj.bias", "attention.k_proj.weight", "attention.k_proj.bias",
          "attention.v_proj.weight", "attention.v_proj.bias", "attention.out_proj.weight", "attention.out_proj.bias",
          "attention.gru_rel_pos_const", "attention.gru_rel_pos_linear.weight", "attention.gru_rel_pos_linear.bias",
          "layer_norm.weight", "layer_norm.bias", "feed_forward.intermediate_dense.weight",
          "feed_forward.intermediate_dense.bias", "feed_forward.output_dense.weight", "feed_forward.output_dense.bias",
          "final_layer_norm.weight", "final_layer_norm.bias"]
_PARENT = {"wavlm-base": (C.WAVLM_BASE, _FRONT_GROUP, 247, 94381168,
                          "74e47e0228bc0869cb25b7f869cd8c719016de98b31fb8774acb1bb60bf40b2e"),
           "wavlm-large": (C.WAVLM_LARGE, _FRONT_LAYER, 487, 315452096,
                           "1f77cc6a7d3b1b2006daba7adef8697b43d8d1ddd73f4d4ed3f8e3204cc94bfb")}


@pytest.mark.parametrize("name", sorted(_PARENT))
def test_named_wavlm_specs_keep_their_order(name):
    spec, front, n, floats, sha = _PARENT[name]
    ps = C.param_specs(spec)
    keys = front + _MIDDLE + [f"encoder.layers.{l}.{k}" for l in range(spec.layers) for k in _LAYER]
    assert [k for k, _ in ps] == keys and len(ps) == n
    assert C.weight_floats(spec) == floats
    assert hashlib.sha256(repr(ps).encode()).hexdigest() == sha


# ---- the fixtures against the unchanged oracle ----------------------------------------------------------------
def test_fixture_inputs_match_manifest():
    man = wf.manifest()
    for name, entries in (("wav2vec2_base", (("emb", "clips_sha256"), ("emb_long", "long_clip_sha256"),
                                             ("hs_short", "short_clip_sha256"))),
                          ("hubert_large4", (("emb", "clips_sha256"), ("hs_short", "short_clip_sha256")))):
        for which, key in entries:
            assert _sha(wf.clips(name, which)) == man[name][key], (name, which)
        h = hashlib.sha256()
        sd = wf.weights(name)
        for k in sorted(sd):
            h.update(k.encode())
            h.update(np.ascontiguousarray(sd[k]).tobytes())
        assert h.hexdigest() == man[name]["weights_sha256"]
    conv_b = [v for k, v in wf.weights("hubert_large4").items()
              if k.startswith("feature_extractor.") and k.endswith(".conv.bias")]
    assert len(conv_b) == 7 and all(np.abs(v).max() > 0 for v in conv_b)     # the conv biases are exercised


def test_wav2vec2_fixture_is_wavlm_with_a_zero_table():
    """oracle/wavlm.py (WavLM, unchanged) on the fixture weights + a zero rel_attn_embed + arbitrary gate tensors
    reproduces what the reference's glue got from transformers' Wav2Vec2Model."""
    from oracle.wavlm import WavLMOracle
    g = wf.golden("wav2vec2_base")
    old, sd = wf.old_route(wf.W2V_SPEC, wf.weights("wav2vec2_base"))
    o = WavLMOracle(old, sd)
    idx = [int(i) for i in g["layer_indices"]]
    assert idx == list(range(13)) and g["emb"].shape == (4, 13, 768)
    assert _rel(o.embed(wf.clips("wav2vec2_base", "emb")[:2], idx), g["emb"][:2]).max() <= ORACLE_TOL
    assert _rel(o.embed(wf.clips("wav2vec2_base", "emb_long"), idx)[0], g["emb_long"]).max() <= ORACLE_TOL
    hs = o.hidden_states(wf.clips("wav2vec2_base", "hs_short")[0])
    assert hs[0].shape == (49, 768)
    for i in (0, 1, 12):
        ref = g[f"hs{i}_short"]
        assert np.linalg.norm(hs[i] - ref) / np.linalg.norm(ref) <= ORACLE_TOL, i


def test_hubert_fixture_is_wavlm_with_a_zero_table():
    """The large shape (conv biases, layer-norm frontend, stable-LN, do_normalize) cut to 4 layers."""
    from oracle.wavlm import WavLMOracle
    g = wf.golden("hubert_large4")
    old, sd = wf.old_route(wf.HUB_SPEC, wf.weights("hubert_large4"))
    o = WavLMOracle(old, sd)
    idx = [int(i) for i in g["layer_indices"]]
    assert idx == list(range(5)) and g["emb"].shape == (3, 5, 1024)
    assert _rel(o.embed(wf.clips("hubert_large4", "emb"), idx, do_normalize=True), g["emb"]).max() <= ORACLE_TOL
    short = wf.clips("hubert_large4", "hs_short")[0]
    hs = o.hidden_states(short, do_normalize=True)
    ref = g["hs0_short"]
    assert hs[0].shape == (49, 1024) and np.linalg.norm(hs[0] - ref) / np.linalg.norm(ref) <= ORACLE_TOL
    # the gate tensors are arbitrary: another draw gives the same function (x + 0 is exact)
    _, sd2 = wf.old_route(wf.HUB_SPEC, wf.weights("hubert_large4"), gate_seed=99)
    assert np.array_equal(WavLMOracle(old, sd2).hidden_states(short, do_normalize=True)[1], hs[1])
