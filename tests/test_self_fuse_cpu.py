"""The plan of the fused QKV + self-attention launch (csrc/attention.hip qkv_attn_kernel; mra_qformer_set_option "self_fuse") and the refusals
of its debug entry, without a GPU: ``mra_debug_self_fuse_plan`` is the predicate run_lanes asks, ``mra_debug_qkv_attention`` refuses every shape
outside the plan and every null or misaligned buffer before anything is launched."""
from mraudio_amd import _lib as L

F16, BF16, F32 = L.MRA_F16, L.MRA_BF16, L.MRA_F32


def _plan(option=1, chain_ring=7, lanes=1, items=32, S=64, hidden=768, heads=12, dtype=F16, want_full=0):
    return L.lib().mra_debug_self_fuse_plan(option, chain_ring, lanes, items, S, hidden, heads, dtype, want_full)


def test_plan_takes_the_fused_launch_only_inside_its_conditions():
    for dt in (F16, BF16):
        for S in (32, 33, 40, 64):
            assert _plan(S=S, dtype=dt) == 1
    assert _plan(items=16) == 1 and _plan(items=17) == 1 and _plan(items=26, S=40) == 1
    assert _plan(items=15) == 0 and _plan(items=3, S=40) == 0      # below 1024 rows the QKV GEMM runs a two-buffer tile: other bits
    assert _plan(chain_ring=6) == 0 and _plan(chain_ring=1) == 1   # ... as it does with the QKV ring tile switched off
    assert _plan(option=0) == 0                       # the option is off
    assert _plan(want_full=1) == 0                    # the full-sequence forward keeps the launches chain_ring selects
    assert _plan(lanes=2) == 0                        # the pair forward keeps the two launches
    assert _plan(S=65) == 0 and _plan(S=192) == 0     # longer prompts (the S = 160 parity case)
    assert _plan(S=0) == 0
    assert _plan(hidden=768, heads=8) == 0            # 96-wide heads
    assert _plan(hidden=768, heads=16) == 0           # 48-wide heads
    assert _plan(dtype=F32) == 0


def _call(rows=1 << 20, w=2 << 20, b=3 << 20, mask=4 << 20, dtype=F16, items=3, S=40, heads=12, ctx=8 << 20):
    return L.lib().mra_debug_qkv_attention(rows, w, b, mask, dtype, items, S, heads, ctx, None)   # never dereferenced: every call is refused


def test_debug_entry_refusals():
    lib = L.lib()
    launched = lib.mra_debug_qkv_attention_launches()
    bad = [_call(S=65), _call(S=160), _call(S=0), _call(heads=0), _call(heads=17), _call(items=-1), _call(dtype=F32),
           _call(rows=None), _call(w=None), _call(ctx=None),
           _call(rows=(1 << 20) + 8), _call(w=(2 << 20) + 8), _call(b=(3 << 20) + 8), _call(ctx=(8 << 20) + 8)]
    assert all(rc == -1 for rc in bad), bad
    assert _call(S=65) == -1 and b"S <= 64" in lib.mra_last_error()
    assert _call(items=0) == 0                        # no items: a no-op after the shape checks
    assert lib.mra_debug_qkv_attention_launches() == launched


def test_option_is_known_and_bounded():
    """set_option needs a handle; the text of the refusal of a null handle shows the entry is reached, the bounds are checked on the GPU."""
    assert L.lib().mra_qformer_set_option(None, b"self_fuse", 1) == -1
