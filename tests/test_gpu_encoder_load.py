"""``-m gpu``: the parameter upload of the encoder handles (``mra_vit_load`` / ``mra_beats_load``, ``*_missing``) through the C ABI, on
small configurations and with no kernel beyond the converts.  The expected counts, return codes and ``mra_last_error`` texts were
recorded from the ``if / else if`` chains these entry points used to be (this file passed against that library unchanged) and pin
the registry that replaced them: ``missing`` counts down to 0 over a fixed upload order, an optional name does not move it, a name
may be loaded twice, and every refusal keeps its code and its words."""
import ctypes as C

import pytest
import torch

from mraudio_amd import _lib

pytestmark = pytest.mark.gpu

EINVAL, ENAME = -1, -5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _load(prefix, h, name, t, numel=None):
    """rc and error text of one ``<prefix>_load``; ``numel`` overrides the shape handed over (the data pointer stays valid)."""
    shape = (C.c_int64 * 1)(t.numel() if numel is None else numel)
    rc = getattr(_lib.lib(), prefix + "_load")(h, name.encode() if name is not None else None, _lib.ptr(t), _lib.mra_dtype(t.dtype), shape, 1,
                                              _lib.current_stream())
    return rc, (_lib.lib().mra_last_error().decode() if rc else "")


def _count_down(prefix, h, names, buf, optional=()):
    missing = getattr(_lib.lib(), prefix + "_missing")
    left = len(names) - len(optional)
    assert missing(h) == left
    for i, (name, n) in enumerate(names):
        t = buf[:n].to((torch.float32, torch.float16, torch.bfloat16)[i % 3])     # every source dtype
        assert _load(prefix, h, name, t) == (0, ""), name
        left -= name not in optional
        assert missing(h) == left, name
    assert missing(h) == 0
    name, n = names[0]
    assert _load(prefix, h, name, buf[:n]) == (0, "") and missing(h) == 0          # a second load of a name is accepted


def _vit_names(depth, D, I, patch, S):
    names = [("cls_token", D), ("pos_embed", S * D), ("patch_embed.weight", D * 3 * patch * patch), ("patch_embed.bias", D)]
    for i in range(depth):
        p = f"blocks.{i}."
        names += [(p + "norm1.weight", D), (p + "norm1.bias", D), (p + "attn.qkv.weight", 3 * D * D), (p + "attn.q_bias", D), (p + "attn.v_bias", D),
                  (p + "attn.proj.weight", D * D), (p + "attn.proj.bias", D), (p + "norm2.weight", D), (p + "norm2.bias", D),
                  (p + "fc1.weight", I * D), (p + "fc1.bias", I), (p + "fc2.weight", D * I), (p + "fc2.bias", D)]
    return names


def test_vit_load_and_missing(dev):
    lib = _lib.lib()
    depth, D, I, patch = 2, 704, 256, 14
    cfg = _lib.mra_vit_cfg(D, 8, I, depth, patch, 2 * patch, 1e-6, _lib.MRA_F16, _lib.MRA_F32)
    h = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(lib.mra_vit_create(C.byref(cfg), C.byref(h)), "mra_vit_create")
        try:
            buf = torch.linspace(-1, 1, 3 * D * D, device=dev)
            names = _vit_names(depth, D, I, patch, 5)
            assert len(names) == 4 + 13 * depth
            one = buf[:D]
            assert _load("mra_vit", h, "blocks.0.norm3.weight", one) == (ENAME, "unknown parameter name: blocks.0.norm3.weight")
            assert _load("mra_vit", h, "blocks.0", one) == (ENAME, "unknown parameter name: blocks.0")
            assert _load("mra_vit", h, "head.weight", one) == (ENAME, "unknown parameter name: head.weight")
            assert _load("mra_vit", h, "blocks.2.norm1.weight", one) == (ENAME, "layer index out of range: blocks.2.norm1.weight")
            assert _load("mra_vit", h, "blocks.-1.norm1.weight", one) == (ENAME, "layer index out of range: blocks.-1.norm1.weight")
            assert _load("mra_vit", h, "blocks.1.fc1.bias", one) == (EINVAL, f"parameter blocks.1.fc1.bias: expected {I} elements, got {D}")
            assert _load("mra_vit", h, "pos_embed", one, numel=7) == (EINVAL, f"parameter pos_embed: expected {5 * D} elements, got 7")
            assert _load("mra_vit", h, None, one) == (EINVAL, "null argument")
            assert lib.mra_vit_load(h, b"cls_token", None, 0, (C.c_int64 * 1)(D), 1, None) == EINVAL and lib.mra_last_error() == b"null argument"
            assert lib.mra_vit_load(h, b"cls_token", _lib.ptr(one), 0, None, 1, None) == EINVAL and lib.mra_last_error() == b"null argument"
            assert lib.mra_vit_load(None, b"cls_token", _lib.ptr(one), 0, (C.c_int64 * 1)(D), 1, None) == EINVAL
            assert lib.mra_vit_load(h, b"cls_token", _lib.ptr(one), 3, (C.c_int64 * 1)(D), 1, None) == EINVAL and lib.mra_last_error() == b"bad dtype"
            assert lib.mra_vit_missing(h) == len(names) and lib.mra_vit_missing(None) == -1     # no refusal counted as a load
            _count_down("mra_vit", h, names, buf)
            torch.cuda.synchronize(dev)
        finally:
            lib.mra_vit_destroy(h)


def _beats_names(layers, D, I, Em, kp, conv_pos, buckets, heads):
    names = [("patch_embedding.weight", Em * kp), ("layer_norm.weight", Em), ("layer_norm.bias", Em), ("post_extract_proj.weight", D * Em),
             ("post_extract_proj.bias", D), ("encoder.pos_conv.0.weight", D * 48 * conv_pos), ("encoder.pos_conv.0.bias", D),
             ("encoder.layer_norm.weight", D), ("encoder.layer_norm.bias", D),
             ("encoder.layers.0.self_attn.relative_attention_bias.weight", buckets * heads)]
    for i in range(layers):
        p = f"encoder.layers.{i}."
        names += [(p + f"self_attn.{x}_proj.weight", D * D) for x in "qkv"] + [(p + f"self_attn.{x}_proj.bias", D) for x in "qkv"]
        names += [(p + "self_attn.out_proj.weight", D * D), (p + "self_attn.out_proj.bias", D), (p + "self_attn.grep_linear.weight", 512),
                  (p + "self_attn.grep_linear.bias", 8), (p + "self_attn.grep_a", heads), (p + "self_attn_layer_norm.weight", D),
                  (p + "self_attn_layer_norm.bias", D), (p + "fc1.weight", I * D), (p + "fc1.bias", I), (p + "fc2.weight", D * I), (p + "fc2.bias", D),
                  (p + "final_layer_norm.weight", D), (p + "final_layer_norm.bias", D)]
    return names


def test_beats_load_and_missing(dev):
    lib = _lib.lib()
    layers, D, I, Em = 2, 768, 256, 256
    cfg = _lib.mra_beats_cfg()
    lib.mra_beats_cfg_default(C.byref(cfg))
    cfg.layers, cfg.ffn, cfg.embed_dim = layers, I, Em
    h = C.c_void_p()
    with torch.cuda.device(dev):
        _lib.check(lib.mra_beats_create(C.byref(cfg), C.byref(h)), "mra_beats_create")
        try:
            buf = torch.linspace(-1, 1, D * 48 * cfg.conv_pos, device=dev)
            names = _beats_names(layers, D, I, Em, cfg.patch * cfg.patch, cfg.conv_pos, cfg.num_buckets, cfg.heads)
            optional = tuple(f"encoder.layers.{i}.self_attn.k_proj.bias" for i in range(layers))
            assert len(names) - len(optional) == 10 + 18 * layers
            one = buf[:D]
            for which in ("weight_g", "weight_v"):
                key = "encoder.pos_conv.0." + which
                assert _load("mra_beats", h, key, one) == (ENAME, key + ": load the effective weight encoder.pos_conv.0.weight (weight norm folded by the caller)")
            assert _load("mra_beats", h, "encoder.layers.1.self_attn.relative_attention_bias.weight", one) == (
                ENAME, "unknown parameter name: encoder.layers.1.self_attn.relative_attention_bias.weight")
            assert _load("mra_beats", h, "encoder.layers.0", one) == (ENAME, "unknown parameter name: encoder.layers.0")
            assert _load("mra_beats", h, "predictor.weight", one) == (ENAME, "unknown parameter name: predictor.weight")
            assert _load("mra_beats", h, "encoder.layers.2.fc1.bias", one) == (ENAME, "layer index out of range: encoder.layers.2.fc1.bias")
            assert _load("mra_beats", h, "encoder.layers.1.fc1.bias", one) == (EINVAL, f"parameter encoder.layers.1.fc1.bias: expected {I} elements, got {D}")
            assert _load("mra_beats", h, "encoder.pos_conv.0.weight", one) == (
                EINVAL, f"parameter encoder.pos_conv.0.weight: expected {D * 48 * cfg.conv_pos} elements, got {D}")
            assert _load("mra_beats", h, None, one) == (EINVAL, "null argument")
            assert lib.mra_beats_load(h, b"layer_norm.bias", None, 0, (C.c_int64 * 1)(Em), 1, None) == EINVAL and lib.mra_last_error() == b"null argument"
            assert lib.mra_beats_load(h, b"layer_norm.bias", _lib.ptr(one), -1, (C.c_int64 * 1)(Em), 1, None) == EINVAL and lib.mra_last_error() == b"bad dtype"
            assert lib.mra_beats_missing(h) == len(names) - len(optional) and lib.mra_beats_missing(None) == -1
            _count_down("mra_beats", h, names, buf, optional)
            torch.cuda.synchronize(dev)
        finally:
            lib.mra_beats_destroy(h)
