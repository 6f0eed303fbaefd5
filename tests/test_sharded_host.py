"""CPU checks of the sharded retrieval layer: host-side argument validation of cmh_topk_merge (nothing is launched), the limits the
binding publishes against the header, the shard / query-block cuts of utils/retrieval.py, and retrieve.py's --index option."""
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT


def test_argument_validation_of_topk_merge():
    import cmh_native as N
    lib = N.lib()
    p = 256                      # a non-null address that is never dereferenced: every call below is refused before any launch
    merge = lambda *, a_idx=p, a_dist=p, a_tag=None, ka=5, b_idx=p, b_dist=p, b_tag=None, kb=7, b_base=100, Q=3, k=6, idx=p, dist=p, \
        tag=None: lib.cmh_topk_merge(a_idx, a_dist, a_tag, ka, b_idx, b_dist, b_tag, kb, b_base, Q, k, idx, dist, tag, None)
    calls = [
        lambda: lib.cmh_topk_merge(None, None, None, 5, None, None, None, 7, 0, 3, 6, None, None, None, None),
        lambda: merge(a_idx=None), lambda: merge(a_dist=None), lambda: merge(b_idx=None), lambda: merge(b_dist=None),
        lambda: merge(idx=None), lambda: merge(dist=None),
        lambda: merge(a_tag=p), lambda: merge(b_tag=p), lambda: merge(tag=p), lambda: merge(a_tag=p, b_tag=p),
        lambda: merge(a_tag=p, tag=p), lambda: merge(b_tag=p, tag=p),
        lambda: merge(k=0), lambda: merge(k=-2), lambda: merge(k=13), lambda: merge(ka=1, kb=1, k=3),
        lambda: merge(ka=0), lambda: merge(kb=0), lambda: merge(ka=-1), lambda: merge(Q=0), lambda: merge(Q=-5),
        lambda: merge(b_base=-1), lambda: merge(Q=65536), lambda: merge(Q=2 ** 31 - 1),
    ]
    for i, call in enumerate(calls):
        rc = call()
        assert rc == -1, (i, rc)
        assert len(lib.cmh_last_error()) > 0
    assert merge(k=13) == -1 and b"k=13" in lib.cmh_last_error()
    assert merge(k=0) == -1 and b"k=0" in lib.cmh_last_error()
    assert merge(b_base=-1) == -1 and b"b_base=-1" in lib.cmh_last_error()
    assert merge(a_tag=p) == -1 and b"tags" in lib.cmh_last_error()
    assert merge(Q=65536) == -1 and b"Q=65536" in lib.cmh_last_error()


def test_limits_of_the_binding_are_the_headers():
    import cmh_native as N
    src = open(os.path.join(ROOT, "include", "cmh.h")).read()
    assert N.TOPK_MAX == int(re.search(r"#define\s+CMH_TOPK_MAX\s+(\d+)", src).group(1)) == 524287
    assert N.QUERIES_MAX == 65535 and re.search(r"Q <= 65535, N <= 524287", src)
    # the entry points themselves still refuse what lies past those limits (the sharding sits above them)
    assert N.lib().cmh_retrieval_workspace_bytes(4, N.TOPK_MAX + 1, 64) == 0
    assert N.lib().cmh_retrieval_workspace_bytes(N.QUERIES_MAX + 1, 100, 64) == 0


def test_topk_merge_binding_refuses_cpu_tensors_and_bad_operands():
    import cmh_native as N
    lst = lambda k, tag=False: (torch.zeros(2, k, dtype=torch.int32), torch.zeros(2, k), torch.zeros(2, k, dtype=torch.uint8) if tag else None)
    with pytest.raises(N.NativeError):
        N.topk_merge(lst(3), lst(4), 10, 5)
    with pytest.raises(N.NativeError):
        N.topk_merge(lst(3)[:2], lst(4), 10, 5)
    with pytest.raises(N.NativeError):
        N.topk_merge(lst(3), (torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 5), None), 10, 5)


def test_cuts_of_shards_and_query_blocks():
    import cmh_native as N
    import utils.retrieval as R
    assert R.SHARD_ITEMS == N.TOPK_MAX
    assert R._cuts(1000, 333) == [(0, 333), (333, 666), (666, 999), (999, 1000)]
    assert R._cuts(1000, 1000) == [(0, 1000)] and R._cuts(7, 1000) == [(0, 7)]
    assert R._cuts(N.QUERIES_MAX + 6, N.QUERIES_MAX) == [(0, 65535), (65535, 65541)]
    z = lambda n: (torch.zeros(n, 1, dtype=torch.int32),) * 2
    Q, n, blocks, shards = R._plan("t", z(9), z(N.TOPK_MAX + 38), None)
    assert (Q, n, blocks) == (9, 524325, [(0, 9)]) and shards == [(0, 524287), (524287, 524325)]
    assert R._plan("t", z(9), z(1000), None)[2:] == ([(0, 9)], [(0, 1000)])              # within the limits: one call, as ever
    t = torch.arange(12, dtype=torch.int32).view(6, 2)
    assert R._rows(t, (0, 6), 6) is t and R._rows(None, (0, 3), 6) is None
    part = R._rows((t, t), (2, 5), 6)
    assert part[0].data_ptr() == t[2:].data_ptr() and part[0].is_contiguous() and part[1].shape == (3, 2)
    for bad in (0, -1, N.TOPK_MAX + 1):
        with pytest.raises(N.NativeError):
            R._plan("t", z(9), z(1000), bad)


def test_retrieve_cli_help_shows_the_index_option():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.join(PKG, "retrieve.py"), "--help"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--index" in out.stdout and "--codes" in out.stdout and "CodeIndex" in out.stdout
