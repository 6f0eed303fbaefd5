"""The plan of every GEMM launch (csrc/gemm.hip: plan_gemm; include/cmh.h: cmh_gemm_plan) against a table recorded from the commit
before the plan existed, when the same decisions were spread over gemm.hip, gemm_wide.hip and gemm_lc.hip (tests/golden/gemm_plan.json
names that commit).  Results never depend on the tile height, the grid, the tile order or the deferred-QuickGELU choice of a launch,
so no other test can see a slip there; this one pins them field by field.  Host-only: nothing is launched, so no GPU is needed (the
plan assumes 256 CUs without one, as on MI355X).

A case is [switch state, dt, epi, a, b, route, launch...]: a / b = [M, N, K, row count on the device, its hint] (b null: a plain
launch), route what cmh_gemm_route says, then per launch [family, tile rows, grid, order group, deferred QuickGELU, residual form,
grouped] (two launches: a grouped request that runs as two plain ones)."""
import json
import os
import subprocess
import sys

import pytest

import cmh_native as N

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = json.load(open(os.path.join(HERE, "golden", "gemm_plan.json")))["cases"]
STATES = sorted({c[0] for c in TABLE if not c[0].startswith("env:")})
ENVS = sorted({c[0][4:] for c in TABLE if c[0].startswith("env:")})
WIDE, ROWS, FALLBACK, LC, LC2, LC3, LC2Q = range(7)
LC_FORM = {WIDE: 0, LC: 1, LC2: 2, LC3: 3}


def _apply(state):
    N.set_gemm_lc(-1)
    N.gemm_tuning(-1, -1)
    N.set_gemm_rows(-1)
    N.set_gemm_grouped(-1)
    if state.startswith("lc="):
        N.set_gemm_lc(int(state[3:]))
    elif state.startswith("tuning="):
        N.gemm_tuning(*map(int, state[7:].split(",")))
    elif state == "rows=0":
        N.set_gemm_rows(0)
    elif state == "grouped=0":
        N.set_gemm_grouped(0)
    else:
        assert state == "default", state


def _plan(case):
    _, dt, epi, a, b = case[:5]
    route, launches = N.gemm_plan(a, b, epi, dt)
    return [route] + [[p[f] for f in N.PLAN_FIELDS] for p in launches]


@pytest.fixture
def switches():
    yield _apply
    _apply("default")


def test_the_table_covers_what_it_is_for():
    assert len(TABLE) <= 4000
    launches = [l for c in TABLE for l in c[6:]]
    assert {l[0] for l in launches} == set(range(7))                              # every kernel family
    assert {l[1] for l in launches if l[0] == WIDE} == {96, 128, 160}             # every tile height of the wide kernel
    assert {len(c) - 6 for c in TABLE} == {1, 2}                                  # one grouped launch, and two plain ones
    assert {l[4] for l in launches} == {0, 1} and {l[5] for l in launches} == {0, 1, 2}
    assert any(l[2] % 8 == 0 and l[2] < 256 for l in launches if l[0] == WIDE)    # fewer tiles than CUs: the grid rounds up to 8
    assert {c[3][0] for c in TABLE} >= {2048, 2049}                               # the few-row kernel's edge
    assert {c[3][2] for c in TABLE} >= {256, 512, 1024, 1088}                     # lc K threshold; 16 / 17 K-steps (residual first)
    assert {c[3][1] // 256 for c in TABLE} >= {3, 4, 11, 12}                      # order-group edges
    assert any(c[3][3] and c[3][4] > c[3][0] for c in TABLE)                      # a hint above M
    assert len(STATES) == 15 and len(ENVS) == 3


@pytest.mark.parametrize("state", STATES)
def test_plan_equals_the_parents(state, switches):
    switches(state)
    cases = [c for c in TABLE if c[0] == state]
    assert cases
    bad = [(c[:5], c[5:], got) for c in cases for got in [_plan(c)] if got != c[5:]]
    assert not bad, f"{len(bad)} of {len(cases)} differ; (case, recorded, got): {bad[:5]}"


_CHILD = """
import json, sys
import cmh_native as N
out = []
for c in json.load(sys.stdin):
    route, launches = N.gemm_plan(c[3], c[4], c[2], c[1])
    out.append([route] + [[p[f] for f in N.PLAN_FIELDS] for p in launches])
print(json.dumps(out))
"""


@pytest.mark.parametrize("env", ENVS)
def test_plan_under_an_environment_switch(env):
    """CMH_GEMM_WIDE / CMH_GEMM_DGE / CMH_GEMM_GROUPED are read once per process: a fresh one"""
    cases = [c for c in TABLE if c[0] == "env:" + env]
    assert len(cases) >= 40
    key, value = env.split("=")
    res = subprocess.run([sys.executable, "-c", _CHILD], input=json.dumps([c[:5] for c in cases]), capture_output=True, text=True,
                         env=dict(os.environ, PYTHONPATH=os.path.dirname(N.__file__), **{key: value}), timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().split("\n")[-1])
    bad = [(c[:5], c[5:], g) for c, g in zip(cases, got) if g != c[5:]]
    assert not bad, f"{len(bad)} of {len(cases)} differ; (case, recorded, got): {bad[:5]}"


@pytest.mark.parametrize("state", STATES)
def test_route_is_the_plans_lc_form(state, switches):
    """cmh_gemm_route on every bf16 case: the plan's route field; and the family of the launch itself wherever the route step alone
    decides it - one launch that reaches the wide kernel's side, no device-side row count (cmh_gemm_route has none to pass), the
    longer K first (cmh_gemm_route takes the problems in the order given)"""
    switches(state)
    cases = [c for c in TABLE if c[0] == state and c[1] == N.BF16]
    assert cases
    for c in cases:
        _, dt, epi, a, b = c[:5]
        route = N.gemm_route(a[:3], None if b is None else b[:3], epi, dt=dt)
        got = _plan(c)
        assert route == got[0] == c[5], c
        if len(got) == 2 and got[1][0] in LC_FORM and not a[3] and not (b and (b[3] or b[2] > a[2])):
            assert LC_FORM[got[1][0]] == route, c
