"""The size of a training tape, pinned: cmh_vit_train_bytes / cmh_text_train_bytes / cmh_blocks_train_bytes are pure host arithmetic
(csrc/encoders_bwd.hip: the carve of a tape over a null base), so nothing is launched here.  tests/golden/train_bytes.json was recorded
from the library of the commit BEFORE the tape's dimensions and its reduction scratch were stated once (TrainDims, BlockRed):

    CMH_LIB=<that library> PYTHONPATH=clip-based-cross-modal-hashing_amd python tests/test_train_bytes_host.py
                                                        (writes the file; never run it on the code under test)

Only the total is pinned; that every slot kept its offset is shown by running one library's backward on a tape the other one filled."""
import ctypes as C
import json
import os

import cmh_native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_bytes.json")
WIDTHS = {128: 64, 256: 128, 768: 512, 1024: 768}          # width -> embed_dim
DTYPES = {"f32": N.F32, "bf16": N.BF16}
BATCHES, LAYERS = (1, 3, 37, 64), (1, 3)
VISION = ((224, 32), (224, 16), (224, 14), (336, 14))       # (resolution, patch); patch 14 in bf16 is the K-padded conv1 (588 -> 768)
TEXT_LENGTHS = (16, 77)
BARE = ((32, 8, 512), (3, 5, 128))                          # (B, T, d)


def measure():
    lib, out = N.lib(), {}
    for dn, dt in DTYPES.items():
        for d, E in WIDTHS.items():
            for layers in LAYERS:
                for B in BATCHES:
                    for res, p in VISION:
                        s = N.VitWeights()
                        s.gemm_dtype, s.resolution, s.patch, s.width, s.layers, s.embed_dim = dt, res, p, d, layers, E
                        out[f"vit/{dn}/r{res}/p{p}/d{d}/l{layers}/b{B}"] = lib.cmh_vit_train_bytes(C.byref(s), B)
                    for L in TEXT_LENGTHS:
                        s = N.TextWeights()
                        s.gemm_dtype, s.context_length, s.vocab_size, s.width, s.layers, s.embed_dim = dt, 77, 49408, d, layers, E
                        out[f"text/{dn}/t{L}/d{d}/l{layers}/b{B}"] = lib.cmh_text_train_bytes(C.byref(s), B, L)
        for B, T, d in BARE:
            for layers in LAYERS:
                out[f"blocks/{dn}/b{B}/t{T}/d{d}/l{layers}"] = lib.cmh_blocks_train_bytes(dt, B, T, d, layers)
    return out


def test_the_grid_is_the_recorded_one():
    got, want = measure(), json.load(open(GOLDEN))
    assert sorted(got) == sorted(want)
    assert len(got) == 2 * (4 * 2 * 4 * (4 + 2) + 2 * 2) and all(v > 0 for v in want.values())
    assert any("/p14/" in k and "/bf16/" in k for k in want)


def test_train_bytes_equal_the_recorded_sizes():
    got, want = measure(), json.load(open(GOLDEN))
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} tape sizes moved, e.g. {sorted(wrong.items())[:4]}"


def test_queries_refuse_bad_arguments_with_zero():
    lib, s, t = N.lib(), N.VitWeights(), N.TextWeights()
    s.gemm_dtype, s.resolution, s.patch, s.width, s.layers, s.embed_dim = N.F32, 224, 0, 128, 1, 64
    assert lib.cmh_vit_train_bytes(C.byref(s), 4) == 0 and lib.cmh_vit_train_bytes(None, 4) == 0
    s.patch = 32
    assert lib.cmh_vit_train_bytes(C.byref(s), 0) == 0
    t.gemm_dtype, t.context_length, t.vocab_size, t.width, t.layers, t.embed_dim = N.F32, 77, 49408, 128, 1, 64
    assert lib.cmh_text_train_bytes(C.byref(t), 0, 16) == 0 and lib.cmh_text_train_bytes(C.byref(t), 4, 0) == 0
    assert lib.cmh_text_train_bytes(None, 4, 16) == 0
    assert lib.cmh_blocks_train_bytes(N.F32, 0, 8, 128, 1) == 0 and lib.cmh_blocks_train_bytes(N.F32, 4, 8, 128, 0) == 0


if __name__ == "__main__":
    sizes = measure()
    with open(GOLDEN, "w") as f:
        json.dump(sizes, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(sizes)} sizes of {N.LIB_PATH} -> {GOLDEN}")
