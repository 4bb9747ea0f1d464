"""Statistics / windowed pooling, host side (no GPU): the segment rule of sse_pool_segments, the torch
route of the drop-in functions (_pool_generic) and the argument checks SSEModel.embed makes before any
device call."""
import numpy as np
import pytest
import torch

POOLINGS = ["mean", "std", "max", "mean_std", "mean_std_max", ("mean", "max"), ("std", "max")]


def _segments(T, win, hop):
    """The rule of include/sse.h, restated: win = 0 is one segment over the clip; a clip of T frames has
    1 segment if T <= win, else 1 + ceil((T - win) / hop); < 0 for arguments the rule rejects."""
    if T < 0 or win < 0:
        return -1
    if win == 0:
        return 1
    if hop <= 0 or win % hop:
        return -1
    if T <= win:
        return 1
    return 1 + -(-(T - win) // hop)


def test_pool_segments_matches_the_rule():
    from ssr_amd import _lib
    seg = _lib.lib().sse_pool_segments
    n = 0
    for win in (0, 1, 4, 8):
        hops = [0] if win == 0 else [h for h in range(1, win + 1) if win % h == 0]
        for hop in hops:
            for T in sorted(set(range(0, 41)) | {win - 1, win, win + 1} - {-1}):
                assert seg(T, win, hop) == _segments(T, win, hop), (T, win, hop)
                n += 1
    assert n > 300
    # the last segment ends at the clip's last frame and every segment is non-empty
    for T, win, hop in [(9, 8, 2), (149, 50, 25), (40, 8, 8), (41, 8, 8), (5, 4, 1)]:
        S = seg(T, win, hop)
        assert (S - 1) * hop < T <= (S - 1) * hop + win
    for bad in [(-1, 0, 0), (10, -1, 1), (10, 4, 0), (10, 4, -2), (10, 4, 3), (10, 8, 16)]:
        assert seg(*bad) < 0, bad


@pytest.mark.parametrize("pooling", POOLINGS)
def test_pool_generic_matches_numpy(pooling):
    from ssr_amd.extract import _pool_generic
    rng = np.random.default_rng(3)
    hs = [torch.from_numpy(rng.standard_normal((1, 7, 8)).astype(np.float32) + 100.0) for _ in range(3)]
    out = _pool_generic(hs, [2, 0, 5], "layer_", pooling)
    assert sorted(out) == ["layer_0", "layer_2"]   # 5 is out of range: reported and skipped, as for the mean
    names = pooling.split("_") if isinstance(pooling, str) else pooling
    for k, i in (("layer_0", 0), ("layer_2", 2)):
        x = hs[i].numpy().astype(np.float64)[0]
        ref = {"mean": x.mean(0), "std": x.std(0, ddof=1), "max": x.max(0)}
        want = np.concatenate([ref[n] for n in ("mean", "std", "max") if n in names])
        got = out[k]
        assert got.dtype == np.float32 and got.shape == (8 * len(names),)
        # fp32 torch against fp64 numpy on values near 100: a few fp32 ulps of 100 (6e-6 each) on every statistic
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)
    if pooling == "mean":
        assert np.array_equal(out["layer_0"], torch.mean(hs[0], dim=1).numpy().flatten())


def test_pool_generic_default_is_the_mean():
    from ssr_amd.extract import _pool_generic
    hs = [torch.arange(24, dtype=torch.float32).reshape(1, 3, 8)]
    assert np.array_equal(_pool_generic(hs, [0], "encoder_layer_")["encoder_layer_0"],
                          torch.mean(hs[0], dim=1).numpy().flatten())


def test_embed_rejects_bad_pooling_before_any_device_call():
    """The checks run first: a handle-less SSEModel (no GPU, no library handle) and no wave are enough."""
    from ssr_amd.model import SSEModel, pool_desc
    m = SSEModel.__new__(SSEModel)
    for kw in [dict(pool="median"), dict(pool="mean_median"), dict(pool=()), dict(pool=("mean", "mean")),
               dict(pool="std_mean"), dict(pool=None), dict(pool="mean_std", window=50),
               dict(pool="mean", hop=25), dict(window=50, hop=20), dict(window=0, hop=1), dict(window=4, hop=0),
               dict(window=-4, hop=2), dict(pool="std", ddof=2)]:
        with pytest.raises(ValueError):
            m.embed(None, [0], **kw)
        with pytest.raises(ValueError):
            pool_desc(**kw)
    d = pool_desc(("max", "mean"), window=50, hop=25, ddof=0, valid_only=True)
    assert (d.stats, d.ddof, d.win, d.hop, d.valid_only) == (5, 0, 50, 25, 1)
    d = pool_desc()
    assert (d.stats, d.ddof, d.win, d.hop, d.valid_only) == (1, 1, 0, 0, 0)


def test_extract_functions_reject_window_and_bad_names():
    from ssr_amd import extract
    with pytest.raises(ValueError):
        extract.extract_embeddings_from_audio_wavlm(np.zeros(16000, np.float32), None, None, "cpu", [0], window=50)
    with pytest.raises(ValueError):
        extract.extract_embeddings_from_audio_whisper(np.zeros(16000, np.float32), None, None, "cpu", [], pooling="rms")
