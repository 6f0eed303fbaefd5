"""query.py::QueryEncoder and retrieve.py --text / --image: captions and pictures -> codes with a checkpoint, equal to what the
trainer's model and its get_code rule give for the same tokenised and preprocessed batch; then the command line end to end on a
saved CodeIndex.  A tiny CLIP with the real vocabulary size (the merges of tests/golden): real BPE ids index its token table."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MERGES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_bpe_merges_48894.txt.gz")
CAPTIONS = ["a dog on a beach", "two people riding bicycles past a red house", "", "a plate of food, with a fork!",
            "an aeroplane above the clouds at sunset " * 4]
BITS, WORDS, RES = 16, 16, 64


def _images():
    rng = np.random.default_rng(5)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((64, 64), (48, 80), (100, 70), (33, 257))]


@pytest.fixture(scope="module")
def clip_file(tmp_path_factory):
    import recipe
    sd = recipe.clip_state_dict(dict(recipe.CLIP_TINY, vocab_size=49408), 7)
    path = tmp_path_factory.mktemp("query") / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    return str(path)


def _trainer_model(method, clip_file, tmp_path):
    """The model as the method's trainer builds it, its heads drawn at random (seeded): -> (model, checkpoint file)."""
    from query import MODELS
    import importlib
    module, name = MODELS[method]
    torch.manual_seed(11)
    kw = dict(outputDim=BITS, clipPath=clip_file, saveDir=str(tmp_path / "log"))
    if method == "DNPH":
        kw["num_classes"] = 24
    model = getattr(importlib.import_module(module), name)(**kw).to(DEV)
    ck = tmp_path / f"{method}.pth"
    torch.save(model.state_dict(), ck)
    model.float()
    model.clip.set_gemm_dtype("f32")
    model.eval()
    return model, str(ck)


@pytest.mark.parametrize("method", ["DSPH", "DCHMT", "DNPH"])
def test_encoder_gives_the_trainers_codes(method, clip_file, tmp_path):
    from code_rules import code_rule
    from dataset.base import shared_tokenizer
    from dataset.gpu_transform import RaggedImages, preprocess
    from query import QueryEncoder
    model, ck = _trainer_model(method, clip_file, tmp_path)
    enc = QueryEncoder(method, ck, clip_file, BITS, max_words=WORDS, resolution=RES, bpe_path=MERGES)
    assert enc.model.clip.assume_frozen is True and enc.bits == BITS
    # the rule the trainer applies for this method (train/base.py::_codes_for_eval) ...
    import cmh_native as N
    # ... restated here, not taken from code_rules.py: DCHMT's argmax over each pair of probabilities, index 0 -> -1, 1 -> +1
    pairs = lambda o: (torch.cat(o, -1).view(o[0].shape[0], -1, 2).argmax(-1) * 2 - 1).float()
    rule = {"DSPH": N.sign_codes, "DCHMT": pairs, "DNPH": lambda o: N.sign_codes(o[0])}[method]
    tokens = shared_tokenizer(MERGES).encode_captions(CAPTIONS, WORDS).to(DEV)
    pixels = preprocess(RaggedImages.from_arrays(_images()).to(DEV), RES, train=False)
    with torch.no_grad():
        want_t, want_i = rule(model.encode_text(tokens)), rule(model.encode_image(pixels))
    got_t, got_i = enc.encode_text(CAPTIONS), enc.encode_image(_images())
    assert tuple(got_t.shape) == (len(CAPTIONS), BITS) and tuple(got_i.shape) == (4, BITS) and got_t.dtype == torch.float32
    assert set(got_t.unique().tolist()) <= {-1.0, 0.0, 1.0} and code_rule(method) is enc.rule
    assert torch.equal(got_t, want_t) and torch.equal(got_i, want_i)
    assert torch.equal(enc.encode_text(CAPTIONS[1]), want_t[1:2]) and torch.equal(enc.encode_image(_images()[2]), want_i[2:3])
    assert len({tuple(r) for r in got_t.tolist()}) > 1              # the captions do not all collapse to one code


def test_retrieve_text_and_image_end_to_end(clip_file, tmp_path):
    from PIL import Image
    from query import QueryEncoder
    from utils.retrieval import CodeIndex
    _, ck = _trainer_model("DSPH", clip_file, tmp_path)
    enc = QueryEncoder("DSPH", ck, clip_file, BITS, max_words=WORDS, resolution=RES, bpe_path=MERGES)
    g = torch.Generator().manual_seed(3)
    db = (torch.randint(0, 2, (300, BITS), generator=g) * 2 - 1).float()
    CodeIndex(db).save(tmp_path / "db.npz")
    picture = tmp_path / "p.png"
    Image.fromarray(_images()[1]).save(picture)
    model = ["--method", "DSPH", "--pretrained", ck, "-clip-path", clip_file, "--output-dim", str(BITS), "--max-words", str(WORDS),
             "--resolution", str(RES), "--bpe-path", MERGES]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--text", CAPTIONS[0], "--image", str(picture), "--text",
                          CAPTIONS[1], "--index", str(tmp_path / "db.npz"), "--k", "10", *model], capture_output=True, text=True,
                         timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 3 * 11
    codes = torch.cat([enc.encode_text(CAPTIONS[0]), enc.encode_image(str(picture)), enc.encode_text(CAPTIONS[1])])
    idx, dist = (t.cpu().numpy() for t in CodeIndex.load(tmp_path / "db.npz").search(codes, 10))
    for i, (kind, value) in enumerate((("text", CAPTIONS[0]), ("image", str(picture)), ("text", CAPTIONS[1]))):
        block = lines[11 * i:11 * i + 11]
        assert block[0] == f"query {i} {kind}: {value}"
        rows = [ln.split() for ln in block[1:]]
        assert [int(r[0]) for r in rows] == list(range(1, 11))
        assert [int(r[1]) for r in rows] == idx[i].tolist() and [float(r[2]) for r in rows] == dist[i].tolist()
    # a model whose code length is not the index's is refused
    bad = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--text", "a dog", "--index", str(tmp_path / "db.npz"),
                          *[a if a != str(BITS) else "32" for a in model]], capture_output=True, text=True, timeout=600, env=env,
                         cwd=str(tmp_path))
    assert bad.returncode != 0 and "16-bit codes" in bad.stderr and "--output-dim 32" in bad.stderr
