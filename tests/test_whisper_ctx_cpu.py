"""Whisper audio context, host side (no GPU, no library call): the frame arithmetic, the validation of the
``frames=`` keyword, and the oracle identity that defines the context's log-mel."""
import numpy as np
import pytest

from ssr_amd import config as C


@pytest.mark.parametrize("n,frames", [(0, 1), (1, 1), (320, 1), (321, 2), (48000, 150), (480000, 1500), (500000, 1500)])
def test_context_frames(n, frames):
    for spec in (C.WHISPER_TINY, C.WHISPER_SMALL, C.WHISPER_LARGE_V2):
        assert spec.context_frames(n) == frames


def _no_library(monkeypatch):
    """Any attempt to load libsse.so fails the test: validation is host arithmetic."""
    from ssr_amd import _lib

    def boom():
        raise AssertionError("frames= validation touched the library")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("bad", [0, 1501, -3, 150.0, "longest", "", True])
def test_frames_validation_raises_before_the_library(monkeypatch, bad):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        C.resolve_frames(C.WHISPER_TINY, bad, 48000)


@pytest.mark.parametrize("frames", [150, 1500, "clip"])
def test_frames_on_a_wavlm_spec_raises(monkeypatch, frames):
    _no_library(monkeypatch)
    with pytest.raises(ValueError):
        C.resolve_frames(C.WAVLM_BASE, frames, 48000)
    assert C.resolve_frames(C.WAVLM_BASE, None, 48000) is None   # the default stays available to every model


def test_frames_resolution():
    s = C.WHISPER_TINY
    assert C.resolve_frames(s, None, 48000) is None
    assert C.resolve_frames(s, 1, 48000) == 1 and C.resolve_frames(s, 1500, 48000) == 1500
    assert C.resolve_frames(s, np.int64(37), 48000) == 37
    assert C.resolve_frames(s, "clip", 48000) == 150
    assert C.resolve_frames(s, "clip", 600000) == 1500
    # "clip" with lengths: the context of the longest clip, whatever the row width
    assert C.resolve_frames(s, "clip", 480000, lengths=[16000, 48001, 7000]) == 151
    assert C.resolve_frames(s, "clip", 480000, lengths=np.array([320, 1])) == 1


def test_model_methods_validate_on_the_host(monkeypatch):
    """SSEModel's methods resolve ``frames`` first: an unbound call with a bad value raises ValueError although
    there is no model, no GPU and no library behind it."""
    _no_library(monkeypatch)
    from ssr_amd import model as M

    def Stub(spec=C.WHISPER_TINY):   # a handle-less instance: nothing was created, nothing is destroyed
        m = object.__new__(M.SSEModel)
        m.spec = spec
        return m
    wave = np.zeros((2, 48000), np.float32)
    for bad in (0, 1501, 2.5, "all"):
        for call in (lambda: M.SSEModel.embed(Stub(), wave, [0], frames=bad),
                     lambda: M.SSEModel.hidden_states(Stub(), wave, frames=bad),
                     lambda: M.SSEModel.whisper_embed(Stub(), wave, [0], [], frames=bad),
                     lambda: M.SSEModel.workspace(Stub(), 2, 48000, frames=bad),
                     lambda: M.SSEModel.pool_segments(Stub(), 48000, frames=bad),
                     lambda: M.logmel(wave, frames=bad)):
            with pytest.raises(ValueError):
                call()
    W = C.WAVLM_BASE
    for call in (lambda: M.SSEModel.embed(Stub(W), wave, [0], frames=150),
                 lambda: M.SSEModel.hidden_states(Stub(W), wave, frames="clip"),
                 lambda: M.SSEModel.workspace(Stub(W), 2, 48000, frames=150)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("F", [150, 160])
def test_oracle_logmel_identity(F):
    """log_mel(w[:320 F])[:, :2F] == log_mel(w)[:, :2F] for a clip that ends inside the context: the zero pad
    starts at the same sample either way, so the context's log-mel is a slice of the usual one -- as long as the
    per-clip maximum of the -8 clamp lies in the kept frames, which holds when the dropped ones are silence."""
    from oracle.whisper import log_mel
    from ssr_amd import synth
    w = synth.synth_clips(1, 48000, seed=9)[0]
    full = log_mel(w)
    cut = log_mel(w[:F * 320])
    assert full.shape == (80, 3000)
    assert np.array_equal(cut[:, :2 * F], full[:, :2 * F])
