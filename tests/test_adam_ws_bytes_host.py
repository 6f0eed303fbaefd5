"""cmh_bert_adam_workspace_bytes (csrc/optim.hip) is a BOUND: it sees only the tensor count and the element total, while the step lays its
tables out from the real chunk count.  Pure host arithmetic - nothing is launched, so this runs without a GPU.

The layout, restated from cmh_bert_adam_step (csrc/optim.hip, "const size_t chunks = adam_chunks(tensors, count)" down to the line that
forms dK), with chunks = sum over tensors of ceil(n / 16384):
    ws  = workspace rounded up to 256 bytes                      (up to 255 bytes lost)
    dT  = ws                                                     sizeof(AdamTensorDev) = 64 bytes per tensor
    dC  = dT + align256(64 * count)                              sizeof(AdamChunk) = 8 bytes per chunk
    dP  = dC + align256(8 * chunks)                              one f32 partial per chunk
    dK  = dP + align256(4 * chunks)                              one f32 coefficient per tensor: the last byte used is dK + 4 * count
The query replaces `chunks` by total / 16384 + count, which is never below it (ceil(n / C) <= floor(n / C) + 1, and a sum of floors is at
most the floor of the sum)."""
import ctypes as C

import cmh_native as N

CHUNK = 16384
SIZES = (49153, 1, 16384, 3, 32769, 4, 16385, 5, 16380, 255, 32768, 256, 16383, 257, 16387, 1023, 1025)   # test_gpu_adam_edges.SIZES
INVALID, WORKSPACE = -1, -2


def a256(x):
    return (x + 255) // 256 * 256


def used(ns):
    chunks = sum((n + CHUNK - 1) // CHUNK for n in ns)
    return 255 + a256(64 * len(ns)) + a256(8 * chunks) + a256(4 * chunks) + 4 * len(ns)


LISTS = {
    "one element": [1],
    "many 1-element tensors": [1] * 1000,
    "257 1-element tensors": [1] * 257,
    "chunk multiples": [CHUNK * k for k in (1, 2, 3, 7, 256, 257)],
    "chunk multiples +- 1": [CHUNK * k + d for k in (1, 2, 5) for d in (-1, 1)],
    "the edge sizes": list(SIZES),
    "one large and many small": [25_000_000] + [1] * 301,
    "32 tensors one short of a chunk": [CHUNK - 1] * 32,
}


def test_struct_sizes_the_layout_counts_with():
    assert C.sizeof(N.AdamTensor) == 64      # cmh_adam_tensor (host ABI); AdamTensorDev has the same fields plus first_chunk in its padding


def test_the_bound_covers_the_layout():
    lib = N.lib()
    for name, ns in LISTS.items():
        got = lib.cmh_bert_adam_workspace_bytes(len(ns), sum(ns))
        assert got >= used(ns), (name, got, used(ns))
        # ... and is tight: what it adds over the layout is the chunks it cannot know are not there (12 bytes each) and the rounding
        spare = sum(ns) // CHUNK + len(ns) - sum((n + CHUNK - 1) // CHUNK for n in ns)
        assert got - used(ns) <= 12 * spare + 3 * 256, (name, got, used(ns), spare)


def test_bad_counts_give_zero():
    lib = N.lib()
    assert lib.cmh_bert_adam_workspace_bytes(0, 10) == 0 and lib.cmh_bert_adam_workspace_bytes(3, 0) == 0
    assert lib.cmh_bert_adam_workspace_bytes(-1, 10) == 0 and lib.cmh_bert_adam_workspace_bytes(3, -5) == 0


def test_refusals_come_before_any_launch():
    """valid shapes, host addresses the call never reads: one byte short is CMH_ERR_WORKSPACE; n = 0, a null stream of data, b1 = 1 and
    b2 = 1 are CMH_ERR_INVALID"""
    lib = N.lib()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p).value
    ns = [5, 16385, 1]
    arr = (N.AdamTensor * len(ns))(*[N.AdamTensor(p, p, p, p, n, 1e-3, 0.2, 1.0, None) for n in ns])
    need = lib.cmh_bert_adam_workspace_bytes(len(ns), sum(ns))
    assert need > 0
    assert lib.cmh_bert_adam_step(arr, len(ns), 0.9, 0.98, 1e-6, p, need - 1, None) == WORKSPACE
    assert b"bert_adam_step: workspace" in lib.cmh_last_error()
    assert lib.cmh_bert_adam_step(arr, len(ns), 1.0, 0.98, 1e-6, p, need, None) == INVALID
    assert lib.cmh_bert_adam_step(arr, len(ns), 0.9, 1.0, 1e-6, p, need, None) == INVALID
    assert lib.cmh_bert_adam_step(arr, len(ns), 0.9, 0.98, -1e-6, p, need, None) == INVALID
    assert lib.cmh_bert_adam_step(arr, 0, 0.9, 0.98, 1e-6, p, need, None) == INVALID
    assert lib.cmh_bert_adam_step(arr, len(ns), 0.9, 0.98, 1e-6, None, need, None) == INVALID
    arr[1].n = 0
    assert lib.cmh_bert_adam_step(arr, len(ns), 0.9, 0.98, 1e-6, p, need, None) == INVALID and b"tensor 1" in lib.cmh_last_error()
    arr[1].n, arr[2].m = 16385, None
    assert lib.cmh_bert_adam_step(arr, len(ns), 0.9, 0.98, 1e-6, p, need, None) == INVALID and b"tensor 2" in lib.cmh_last_error()
