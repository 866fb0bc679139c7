"""CPU-side checks of the shared pre-LN encoder block (walkgpt_amd/encoder_block.py): every GEMM chain's derived operands are keyed on
the tensors that chain reads -- an in-place edit of one of them changes the key, an edit of a tensor the chain does not read leaves it.
The builders themselves need the GPU and are not called: a stub stands in for them behind the same _prep_get, deps and slot."""
from types import SimpleNamespace

import pytest
import torch

from walkgpt_amd.clip_encoder import _EncoderLayer
from walkgpt_amd.segment_anything.modeling import Block


def _sam_block():
    return Block(dim=64, num_heads=2, use_rel_pos=True, window_size=14, input_size=(32, 32)).bfloat16()


def _clip_layer():
    return _EncoderLayer(SimpleNamespace(hidden_size=64, intermediate_size=256, num_attention_heads=2, layer_norm_eps=1e-5)).bfloat16()


def _key(blk, chain, built):
    """The chain's cache key after a _prep_get with the chain's own deps and slot; `built` counts the rebuilds."""
    slot = blk._SLOTS[chain]
    blk._prep_get(lambda: built.append(chain), blk._chain_deps(chain, blk._parts()), slot=slot)
    return getattr(blk, "_prep_key" + slot)


def _edit(t):
    with torch.no_grad():
        t.add_(1)


# chain -> (a tensor of its dep list, a tensor it does not read); the qkv operand is SAM's parameter and CLIP's concatenation of three
_SAM = {"bf16": (lambda b: b.norm2.bias, lambda b: b.attn.proj.weight),
        "mx": (lambda b: b.attn.proj.weight, lambda b: b.attn.proj.bias),
        "fp8": (lambda b: b.mlp.lin2.weight, lambda b: b.norm1.weight)}
_CLIP = {"bf16": (lambda l: l.self_attn.k_proj.bias, lambda l: l.self_attn.out_proj.weight),
         "mx": (lambda l: l.mlp.fc2.weight, lambda l: l.mlp.fc2.bias),
         "fp8": (lambda l: l.self_attn.v_proj.weight, lambda l: l.layer_norm2.weight)}


@pytest.mark.parametrize("make,cases", [(_sam_block, _SAM), (_clip_layer, _CLIP)], ids=["sam", "clip"])
@pytest.mark.parametrize("chain", ["bf16", "mx", "fp8"])
def test_chain_key_follows_the_tensors_the_chain_reads(make, cases, chain):
    blk = make()
    read, unread = (f(blk) for f in cases[chain])
    built = []
    k0 = _key(blk, chain, built)
    assert _key(blk, chain, built) == k0 and built == [chain]            # nothing moved: no rebuild
    _edit(unread)
    assert _key(blk, chain, built) == k0 and built == [chain]
    _edit(read)
    assert _key(blk, chain, built) != k0 and built == [chain, chain]
    others = [c for c in cases if c != chain]
    assert all(getattr(blk, "_prep_key" + blk._SLOTS[c], None) is None for c in others)   # the slots are keyed independently


def test_prepare_and_dispatch_pick_the_chain_from_gemm_dtype_then_widths():
    blk = _sam_block()                     # D = 64: no MX chain
    assert blk._chain(blk._parts()) == "bf16"
    blk.gemm_dtype = "fp8"
    assert blk._chain(blk._parts()) == "fp8"
    wide = Block(dim=256, num_heads=4, use_rel_pos=True, window_size=14, input_size=(32, 32))
    wide.gemm_dtype = "fp8"
    assert wide._chain(wide._parts()) == "mx"
