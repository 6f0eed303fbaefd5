"""The Python layer between the models and libcmh's tower entry points (model/base/model.py, mith_ops.py): a public call walks
each tower's parameters at most once (never when frozen), the prefetched pair is the two separate calls, and the one bf16 copy of
a GEMM weight lives and dies with its parameter."""
import gc
import weakref

import pytest
import torch

import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = recipe.CLIP_TINY


@pytest.fixture(scope="module")
def model():
    from model.base.model import CLIP
    torch.manual_seed(5)
    m = CLIP(**CFG).to(DEV).float().set_gemm_dtype("bf16")
    img = torch.from_numpy(recipe.images(4, CFG["image_resolution"], 1)).to(DEV)
    txt = torch.from_numpy(recipe.captions(4, 16, CFG["vocab_size"], 2)).to(DEV)
    return m, img, txt


@pytest.fixture
def scans(monkeypatch):
    """counts the calls of the one function that walks a tower's parameters, per tower"""
    from model.base.model import CLIP
    count, scan = {"vit": 0, "text": 0}, CLIP._scan

    def counting(self, tower):
        count[tower.name] += 1
        return scan(self, tower)
    monkeypatch.setattr(CLIP, "_scan", counting)
    return count


def test_a_public_call_scans_each_tower_at_most_once(model, scans):
    m, img, txt = model
    calls = {"encode_image": (lambda: m.encode_image(img), {"vit": 1, "text": 0}),
             "encode_text": (lambda: m.encode_text(txt), {"vit": 0, "text": 1}),
             "encode_text(mask)": (lambda: m.encode_text(txt, key_padding_mask=(txt == 0)), {"vit": 0, "text": 1}),
             "encode_pair": (lambda: m.encode_pair(img, txt), {"vit": 1, "text": 1}),
             "prefetch_pair": (lambda: m.prefetch_pair(img, txt), {"vit": 1, "text": 1}),
             "pick-up image": (lambda: m.encode_image(img), {"vit": 1, "text": 0}),
             "pick-up text": (lambda: m.encode_text(txt), {"vit": 0, "text": 1})}
    with torch.no_grad():
        for frozen in (False, True):
            m.assume_frozen = frozen
            m.drop_pair_stash()
            for name, (call, most) in calls.items():
                scans.update(vit=0, text=0)
                call()
                for tower in ("vit", "text"):
                    assert scans[tower] <= (0 if frozen else most[tower]), (name, frozen, dict(scans))
            assert not m._pair_stash                                  # both pick-ups were served from the stash
    m.assume_frozen = False


def test_the_first_call_after_an_update_scans_once_and_sees_it(model, scans):
    m, img, txt = model
    with torch.no_grad():
        before = m.encode_image(img).clone()
        m.visual.proj.mul_(2.0)
        scans.update(vit=0, text=0)
        after = m.encode_image(img)
        assert scans == {"vit": 1, "text": 0} and not torch.equal(before, after)
        m.visual.proj.mul_(0.5)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_prefetch_pair_hands_out_the_separate_calls_features(model, mode):
    m, img, txt = model
    m.set_gemm_dtype(mode)
    with torch.no_grad():
        for pack in (True, False):
            m.pack_text = pack
            ref = m.encode_image(img).clone(), m.encode_text(txt).clone()
            m.prefetch_pair(img, txt)
            assert set(m._pair_stash) == {"image", "text"}
            got = m.encode_text(txt), m.encode_image(img)
            assert not m._pair_stash and torch.equal(got[1], ref[0]) and torch.equal(got[0], ref[1])
    del m.pack_text
    m.set_gemm_dtype("bf16")


def test_training_forward_keeps_what_its_struct_points_at(model):
    """the tape's struct outlives a rebuild of the cache: after an encode in the other mode has put a new entry in the cache, the
    backward still reads the weights its forward ran with (the ctx holds the cache entry's `keep` list and block array)"""
    m, img, _ = model
    m.zero_grad(set_to_none=True)
    f = m.encode_image(img)
    held = f.grad_fn.held
    assert held is m._tower_cache["vit"] and held.keep and held.blocks is not None
    with torch.no_grad():
        m.set_gemm_dtype("f32").encode_image(img)                     # another entry takes the cache's place
    assert m._tower_cache["vit"] is not held and f.grad_fn.held is held
    f.sum().backward()
    g0 = m.visual.proj.grad.clone()
    m.zero_grad(set_to_none=True)
    m.set_gemm_dtype("bf16").encode_image(img).sum().backward()
    assert torch.equal(g0, m.visual.proj.grad)
    m.zero_grad(set_to_none=True)


def test_bf16_gemm_sees_an_in_place_weight_update():
    import cmh_native as N
    import mith_ops as M
    g = torch.Generator().manual_seed(9)
    x = torch.randn(70, 128, generator=g).to(DEV)
    w = torch.nn.Parameter(torch.randn(128, 128, generator=g).to(DEV))       # the GEMM's tile: N % 128, K % 128
    y0 = M.gemm(x, w, dtype=N.BF16)
    assert M.weight_bf16(w) is M.weight_bf16(w)                       # one copy, reused while the weight stands
    with torch.no_grad():
        w.mul_(-2.0)
    y1 = M.gemm(x, w, dtype=N.BF16)
    fresh = torch.nn.Parameter(w.detach().clone())                    # the same values in a weight that never had a copy
    assert torch.equal(y1, M.gemm(x, fresh, dtype=N.BF16)) and not torch.equal(y1, y0)
    assert torch.equal(M.weight_bf16(w), w.detach().to(torch.bfloat16))


def test_bf16_copy_dies_with_its_parameter():
    import cmh_native as N
    import mith_ops as M
    x = torch.randn(8, 128, device=DEV)
    w = torch.nn.Parameter(torch.randn(128, 128, device=DEV))
    M.gemm(x, w, dtype=N.BF16)
    copy = weakref.ref(M.weight_bf16(w))
    assert copy() is not None
    del w
    gc.collect()
    assert copy() is None
