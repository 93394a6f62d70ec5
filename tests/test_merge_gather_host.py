"""The merge launch's entries as far as no GPU is needed: the exported names, the slot mirror's layout, that merge_frames picks the
weight columns merge picks, and that denoise_svd stands as it did."""
import ctypes
import inspect

import pytest
import torch

import helpers  # noqa: F401


def test_new_names_are_exported():
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import _lib, ops
    for name in ("denoise_svd", "DenoiseLoop"):
        assert callable(getattr(P, name)), name
    for name in ("merge_gather", "merge_gather_launch_shape"):
        assert callable(getattr(ops, name)), name
    assert callable(P.ControlNetRouter.merge_frames) and callable(P.ControlNetRouter.merge)
    lib = _lib.lib()
    for name in ("ctrl_op_merge_gather_group", "ctrl_op_merge_gather_launch_shape"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.ctrl_abi_version() == 11                  # symbols were added, nothing changed
    # the slot mirror has the header's layout: 8 pointers, a pointer, an int64 and two int32
    assert ctypes.sizeof(_lib.MergeSlot) == 8 * 8 + 8 + 8 + 4 + 4 and _lib.MERGE_SLOTS == 13
    assert _lib.MergeSlot.out.offset == 64 and _lib.MergeSlot.elems.offset == 72 and _lib.MergeSlot.row.offset == 80


def test_denoise_svd_keeps_its_signature():
    import ctrl_adapter_amd as P
    assert list(inspect.signature(P.denoise_svd).parameters) == [
        "controlnet", "adapter", "unet", "scheduler", "latents", "image_latents", "image_embeddings", "added_time_ids",
        "controlnet_prompt_embeds", "images", "num_inference_steps", "min_guidance_scale", "max_guidance_scale",
        "controlnet_conditioning_scale", "control_guidance_start", "control_guidance_end", "fixed_controlnet_timestep", "skip_conv_in",
        "skip_time_emb", "guess_mode", "sparse_frames", "graph"]


def test_denoise_svd_still_refuses_sparse_frames():
    import ctrl_adapter_amd as P
    with pytest.raises(ValueError, match="sparse_frames"):
        P.denoise_svd(None, None, None, None, torch.zeros(1, 4, 4, 8, 8), None, None, None, None, None, sparse_frames=[0])


def test_merge_frames_reads_the_weight_columns_merge_reads(monkeypatch):
    """merge and merge_frames each compute the active experts' weight columns (quirk N6 and train.py's formula); recorded at the op
    each of them calls, they agree"""
    import ctrl_adapter_amd as P
    from ctrl_adapter_amd import ops
    got = {}
    monkeypatch.setattr(ops, "router_merge", lambda experts, w, widx: got.setdefault("merge", (len(experts), list(widx))) and None)

    def fake_gather(slots, weights, rows, widx, frame_map=None, out_dtype=None):
        got["frames"] = (len(slots[0]), list(widx))
        assert rows == list(range(len(slots))) and tuple(weights.shape) == (13, len(masks))
        return [None] * len(slots)
    monkeypatch.setattr(ops, "merge_gather", fake_gather)
    for masks, nf in (([1, 0, 1], 4), ([1, 1, 1], 2), ([0, 1, 1, 1, 0, 1], 2), ([1, 1], 1), ([1, 0], 16)):
        for quirk in (True, False):
            k = sum(masks)
            w = torch.zeros(13, len(masks))
            downs, mids = [[None] * 12 for _ in range(k)], [None] * k
            got.clear()
            P.ControlNetRouter.merge(downs, mids, w[:12], w[12], masks, num_frames=nf, inference_quirk=quirk)
            d, m = P.ControlNetRouter.merge_frames(downs, mids, w[:12], w[12], masks, num_frames=nf, inference_quirk=quirk)
            assert got["merge"] == got["frames"], (masks, nf, quirk, got)
            assert got["frames"][1] == ([e // nf for e in range(len(masks)) if masks[e]] if quirk else list(range(k)))
            assert len(d) == 12
    with pytest.raises(ValueError, match="num_frames"):
        P.ControlNetRouter.merge_frames([[None] * 12], [None], torch.zeros(12, 2), torch.zeros(2), [1, 0])
