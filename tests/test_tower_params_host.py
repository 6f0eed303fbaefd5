"""Host checks (no GPU) of the towers' parameter tables (model/base/train_ops.py): the tables follow the ctypes structs field for
field, the parameter lists derived from them are the lists written here by hand, they cover each tower exactly, and the cache key
made of them moves when, and only when, it should."""
import pytest
import torch

import recipe

UNEQUAL = dict(recipe.CLIP_TINY, vision_layers=3, transformer_layers=3, vision_width=192, transformer_width=64, transformer_heads=1)


@pytest.fixture(scope="module", params=[recipe.CLIP_TINY, UNEQUAL], ids=["tiny", "3-blocks-unequal-widths"])
def clip(request):
    from model.base.model import CLIP
    torch.manual_seed(11)
    return CLIP(**request.param).float()


def _block_by_hand(blk):
    return [blk.attn.in_proj_weight, blk.attn.in_proj_bias, blk.attn.out_proj.weight, blk.attn.out_proj.bias,
            blk.ln_1.weight, blk.ln_1.bias, blk.ln_2.weight, blk.ln_2.bias,
            blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias]


def _vit_by_hand(v):
    head = [v.conv1.weight, v.class_embedding, v.positional_embedding, v.ln_pre.weight, v.ln_pre.bias,
            v.ln_post.weight, v.ln_post.bias, v.proj]
    return head + [p for blk in v.transformer.resblocks for p in _block_by_hand(blk)]


def _text_by_hand(clip):
    head = [clip.token_embedding.weight, clip.positional_embedding, clip.ln_final.weight, clip.ln_final.bias,
            clip.text_projection]
    return head + [p for blk in clip.transformer.resblocks for p in _block_by_hand(blk)]


def _same(got, want):
    return len(got) == len(want) and all(a is b for a, b in zip(got, want))


def test_block_table_is_the_structs_field_order():
    import cmh_native as N
    from model.base import train_ops as T
    fields = [f for f, *_ in T.BLOCK_TABLE]
    assert fields == [f for f, _ in N.BlockGrads._fields_]
    assert fields == [f for f, _ in N.BlockWeights._fields_][:12]
    assert [f for f, _, gemm in T.BLOCK_TABLE if gemm] == ["in_proj_w", "out_proj_w", "fc_w", "proj_w"]
    # the fp8 mode's per-channel scales sit in the `*_cs` field next to each GEMM weight
    assert [f[:-1] + "cs" for f, _, gemm in T.BLOCK_TABLE if gemm] == [f for f, _ in N.BlockWeights._fields_][12:16]


def test_head_tables_are_the_structs_field_order():
    import cmh_native as N
    from model.base import train_ops as T
    for tower, n in ((T.VIT, 8), (T.TEXT, 5)):
        assert len(tower.head) == n and max(tower.first) == n - 1
        assert [g for _, g, *_ in tower.head] + ["blocks"] == [f for f, _ in tower.grads._fields_]
        weights = [f for f, t in tower.weights._fields_]
        assert [w for w, *_ in tower.head] == weights[6:6 + n] and weights[6 + n:] == ["blocks"]
        assert set(tower.geometry(tower.root(_tiny_clip()))) | {"gemm_dtype", "layers"} == set(weights[:6])
        # only the output projection goes over transposed, and it is a GEMM weight
        assert [(w, g) for w, g, _, gemm in tower.head if w != g] == [(tower.head[-1][0], tower.head[-1][1])] and tower.head[-1][3]
    assert (N.VitGrads, N.TextGrads, N.VitWeights, N.TextWeights) == (T.VIT.grads, T.TEXT.grads, T.VIT.weights, T.TEXT.weights)


def _tiny_clip():
    from model.base.model import CLIP
    return CLIP(**recipe.CLIP_TINY)


def test_parameter_lists_are_the_lists_written_by_hand(clip):
    import mith_train_ops
    from model.base import train_ops as T
    assert _same(T.vit_params(clip.visual), _vit_by_hand(clip.visual)) and _same(T.VIT.params(clip), _vit_by_hand(clip.visual))
    assert _same(T.text_params(clip), _text_by_hand(clip)) and _same(T.TEXT.params(clip), _text_by_hand(clip))
    blocks = clip.transformer.resblocks
    assert _same(T.block_params(blocks[0]), _block_by_hand(blocks[0]))
    assert _same(mith_train_ops.blocks_params(blocks), [p for b in blocks for p in _block_by_hand(b)])
    assert T.VIT.projection(clip) is clip.visual.proj and T.TEXT.projection(clip) is clip.text_projection


def test_the_two_lists_cover_the_module_once_except_logit_scale(clip):
    from model.base import train_ops as T
    listed = [id(p) for p in T.vit_params(clip.visual) + T.text_params(clip)]
    assert len(listed) == len(set(listed))
    assert set(listed) == {id(p) for n, p in clip.named_parameters() if n != "logit_scale"}
    assert {id(p) for p in T.vit_params(clip.visual)} == {id(p) for p in clip.visual.parameters()}
    assert len(list(clip.parameters())) == len(listed) + 1


def test_block_grads_point_at_the_gradient_of_the_same_row(clip):
    """_block_grads (the towers' and the bare stack's) hands field f of block i the gradient of that block's parameter f"""
    from model.base import train_ops as T
    params = T.text_params(clip)
    grads = [torch.empty_like(p) for p in params]
    arr = T._block_grads(grads, len(T.TEXT.head))
    bare = T._block_grads(grads[len(T.TEXT.head):])
    for i, blk in enumerate(clip.transformer.resblocks):
        for j, (field, get, _) in enumerate(T.BLOCK_TABLE):
            g = grads[len(T.TEXT.head) + 12 * i + j]
            assert g.shape == get(blk).shape and getattr(arr[i], field) == g.data_ptr() == getattr(bare[i], field)


def test_key_moves_with_the_weights_and_the_mode_and_not_when_frozen(clip):
    from model.base import train_ops as T
    for tower, p in ((T.VIT, clip.visual.transformer.resblocks[-1].mlp.c_proj.bias), (T.TEXT, clip.token_embedding.weight)):
        other = T.TEXT if tower is T.VIT else T.VIT
        clip.assume_frozen = False
        clip.set_gemm_dtype("f32")
        k0, o0 = clip._key(tower), clip._key(other)
        assert clip._key(tower) == k0
        with torch.no_grad():
            p.add_(1.0)
        k1 = clip._key(tower)
        assert k1 != k0 and clip._key(other) == o0                 # this tower's key only
        clip.set_gemm_dtype("bf16")
        k2 = clip._key(tower)
        assert k2 != k1 and k2[2] == k1[2]                         # the mode moved, the scan did not
        clip.assume_frozen = True
        f0 = clip._key(tower)
        with torch.no_grad():
            p.add_(1.0)
        assert clip._key(tower) == f0 and f0 != k2
        clip.set_gemm_dtype("f32")
        assert clip._key(tower) != f0                              # the mode still counts when frozen
        clip.assume_frozen = False
        assert clip._key(tower)[2] == clip._scan(tower) != k2[2]


def test_frozen_means_no_scan_at_all(clip, monkeypatch):
    from model.base import train_ops as T
    from model.base.model import CLIP
    calls = []
    scan = CLIP._scan
    monkeypatch.setattr(CLIP, "_scan", lambda self, tower: calls.append(tower.name) or scan(self, tower))
    clip.assume_frozen = True
    clip._key(T.VIT), clip._key(T.TEXT), clip._versions(T.VIT)
    assert calls == []
    clip.assume_frozen = False
    clip._key(T.VIT), clip._key(T.TEXT, versions=clip._versions(T.TEXT))
    assert calls == ["vit", "text"]


def test_both_build_models_infer_one_set_of_shapes():
    from model import MITH
    from model.base.model import CLIP, build_model, infer_shapes
    for cfg in (recipe.CLIP_TINY, UNEQUAL):
        sd = lambda: {k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(cfg, 7).items()}
        want = dict(cfg, transformer_heads=cfg["transformer_width"] // 64)
        assert infer_shapes(sd()) == want
        a, b = build_model(sd()), MITH.build_model(sd())
        assert type(a) is CLIP and type(b) is MITH.CLIP1
        assert [(n, tuple(p.shape)) for n, p in a.named_parameters()] == [(n, tuple(p.shape)) for n, p in b.named_parameters()]
    with pytest.raises(NotImplementedError, match="only ViT CLIP checkpoints"):
        MITH.build_model({"text_projection": torch.zeros(2, 2)})
