"""DDWSH on the GPU (csrc/dws.hip through train/DDWSH): the margin loss, its count and the three gradients against the REFERENCE's own
values and autograd gradients on the triplets the reference drew (tests/golden/make_golden23.py), handed in; the sampler against the
float64 restatement of tests/ddwshutil.py taking its inverse-cdf pick ON THE KERNEL'S OWN weights; the weights against the restatement on
the kernel's own distances and against the reference's recorded q; edge shapes; bit-equality; the trainer end to end, a three-step
training trajectory against the reference's, and the query front end.  Tolerances are those of tests/test_gpu_msch.py /
tests/test_gpu_dscph.py: rtol 2e-4, atol 2e-5 of the reference's maximum.  Nothing here claims anything about mAP.

How a negative pick is compared exactly.  The kernel writes the weights it samples from; the restatement forms their ascending running
sum in float64 and picks the first item above u total.  The kernel's sum has the same order, so the two agree unless u total lies
within rounding of a boundary: an anchor is compared only when it lies at least 1e-9 total from every boundary, and at most 1 % of a
case's anchors may be left out that way (tests/test_ddwsh_host.py checks the committed uniforms against that cap on the CPU)."""
import numpy as np
import pytest
import torch

import ddwshutil as dw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN_TAGS = [f"B{B}_K{K}_C{Cn}" for B, K, Cn, _, _ in dw.CASES]
TAGS = GOLDEN_TAGS + [c["tag"] for c in dw.special_cases()]
LAST = np.nextafter(np.float32(1), np.float32(0))
tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
ti = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
num = lambda a: a.detach().cpu().numpy()


def _close(got, ref, what):
    got, ref = np.asarray(num(got) if torch.is_tensor(got) else got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    print(f"{what}: max |diff| {np.abs(got - ref).max():.3e} of max |ref| {top:.3e}")
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-5 * top, err_msg=str(what))


def _case(tag):
    return {c["tag"]: c for c in dw.all_cases()}[tag]


def _three(c):
    """the step's three pairs as device tensors: (x, x), (y, y), (x, y), with `v is u` on the intra-modal ones"""
    x, y = tt(c["x"]), tt(c["y"])
    return [(x, x), (y, y), (x, y)]


def _loss(pairs, c, trips, scale=2.0):
    """native forward and backward on given triplets -> loss [n], count [n], [(du, dv)], dbeta, dist (numpy but for the gradient tensors)"""
    import cmh_native as N
    loss, count, dist, saved = N.dws_margin_loss(pairs, tt(c["lab"]), tt(c["beta"]), ti(trips), dw.MARGIN)
    grads, dbeta = N.dws_margin_loss_backward(saved, torch.full((len(pairs),), scale, device=DEV))
    return num(loss).astype(np.float64), num(count), grads, dbeta, num(dist)


def _q(w):
    tot = w.sum(1, keepdims=True)
    return w / np.where(tot > 0, tot, 1.0)


def _mine(pairs, c, uni, space="distances", cutoff=dw.CUTOFF):
    """-> triplets [n, B, 2], weights f64 [n, B, B], dist f32 [n, B, B] (numpy) of one sampler call"""
    import cmh_native as N
    dist, (ops, _, _) = N.dws_distances(pairs)
    trip, w = N.dws_mine(dist, tt(c["lab"]), ops[0][0].shape[1], tt(uni), cutoff, space, weights=True)
    return num(trip), num(w), num(dist)


def _check_sampler(c, trip, w, uni, what):
    """every valid flag and positive pick against the restatement, every negative pick against the restatement's inverse-cdf pick on the
    kernel's own weights (the skip rule of the module docstring) -> the number of anchors left out"""
    pos, valid = dw.positives(c["lab"])
    B = len(valid)
    skipped = 0
    for q in range(trip.shape[0]):
        assert np.array_equal(trip[q, :, 0] >= 0, valid) and np.array_equal(trip[q, :, 1] >= 0, valid), (what, q)
        assert not w[q][~valid].any() and not w[q][pos].any() and (w[q] >= 0).all() and (w[q] <= 1).all(), (what, q)
        for i in np.flatnonzero(valid):
            assert trip[q, i, 0] == dw.pick_positive(pos[i], i, uni[q, i, 0]), (what, q, i)
            j, margin = dw.pick_negative(w[q, i], uni[q, i, 1])
            assert w[q, i, trip[q, i, 1]] > 0, (what, q, i)                          # an item of weight 0 is never picked
            if margin < 1e-9:
                skipped += 1
                continue
            assert trip[q, i, 1] == j, (what, q, i, trip[q, i, 1], j, margin)
        assert skipped <= 0.01 * B * (q + 1), (what, skipped)
    return skipped


@pytest.mark.parametrize("tag", TAGS)
def test_loss_count_and_gradients_match_reference(golden, tag):
    g = golden("ddwsh.npz")
    c = _case(tag)
    x, y = tt(c["x"]), tt(c["y"])
    for mode, pair in (("intra", (x, x)), ("cross", (x, y))):
        key = f"{tag}_{mode}"
        loss, count, grads, dbeta, dist = _loss([pair], c, g[f"{key}_trip"][None])
        assert int(count[0]) == int(g[f"{key}_count"]), (key, count, int(g[f"{key}_count"]))
        _close(loss, np.array([float(g[f"{key}_loss"])]), (key, "loss"))
        du, dv = grads[0]
        assert (dv is None) == (mode == "intra")                                     # an intra-modal pair: the whole gradient in du
        if int(g[f"{key}_count"]) == 0:
            assert loss[0] == 0.0 and not du.any() and not dbeta.any() and (dv is None or not dv.any())
            continue
        _close(du, 2.0 * g[f"{key}_gx"].astype(np.float64), (key, "gx"))
        if mode == "cross":
            _close(dv, 2.0 * g[f"{key}_gy"].astype(np.float64), (key, "gy"))
        _close(dbeta, 2.0 * g[f"{key}_gbeta"].astype(np.float64), (key, "gbeta"))
        if mode == "intra":
            assert (np.diag(dist[0]) == np.float32(1e-8)).all()                      # the direct difference form: exactly the clamp


@pytest.mark.parametrize("tag", TAGS[:-1])
def test_step_through_the_module_matches_reference(golden, tag):
    """MarginLoss.forward with the step's recorded triplets handed in: one autograd function around the three pairs"""
    from train.DDWSH.loss import MarginLoss
    g = golden("ddwsh.npz")
    c = _case(tag)
    fn = MarginLoss(c["lab"].shape[1]).to(DEV)
    fn.beta.data.copy_(tt(c["beta"]))
    out = []
    for _ in range(2):
        hi, ht = tt(c["x"]).requires_grad_(), tt(c["y"]).requires_grad_()
        fn.beta.grad = None
        with torch.no_grad():
            plain = fn(hi, ht, tt(c["lab"]), ti(g[f"{tag}_step_trips"]))
        loss = fn(hi, ht, tt(c["lab"]), ti(g[f"{tag}_step_trips"]))
        assert loss.dim() == 0 and torch.equal(plain, loss.detach())
        (2.0 * loss).backward()
        out.append((loss.detach().clone(), hi.grad, ht.grad, fn.beta.grad.clone()))
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))                    # two identical calls: bit-equal
    _close(out[0][0].reshape(1), np.array([float(g[f"{tag}_step_loss"])]), (tag, "step loss"))
    for name, mine, key in zip(("gi", "gt", "gbeta"), out[0][1:], ("step_gi", "step_gt", "step_gbeta")):
        _close(mine, 2.0 * g[f"{tag}_{key}"].astype(np.float64), (tag, name))


@pytest.mark.parametrize("space", dw.SPACES)
@pytest.mark.parametrize("tag", TAGS)
def test_sampler_picks_are_the_inverse_cdf_on_its_own_weights(tag, space):
    c = _case(tag)
    B = c["x"].shape[0]
    uni = dw.case_uniforms(3, B, c["seed"])
    trip, w, _ = _mine(_three(c), c, uni, space)
    print(f"{tag} {space}: {_check_sampler(c, trip, w, uni, (tag, space))} anchors within 1e-9 of a cdf boundary")
    # the edge uniforms: u = 0 -> the first item of positive weight; u = nextafter(1, 0) = 1 - 2^-24 -> the last one, unless the
    # items behind the inverse-cdf pick hold less than 2^-24 of the mass together (the pick is then the restatement's, with no skip:
    # u total is a float32 fraction away from every boundary it is compared with)
    for u, side in ((np.float32(0), 0), (LAST, -1)):
        edge = np.full((3, B, 2), u, np.float32)
        trip_e, w_e, _ = _mine(_three(c), c, edge, space)
        assert np.array_equal(w_e, w)
        pos, valid = dw.positives(c["lab"])
        for q in range(3):
            for i in np.flatnonzero(valid):
                have = np.flatnonzero(w[q, i] > 0)
                assert trip_e[q, i, 1] == dw.pick_negative(w[q, i], u)[0], (tag, space, q, i, float(u))
                if side == 0 or w[q, i, have[-1]] > 2.0 ** -23 * w[q, i].sum():
                    assert trip_e[q, i, 1] == have[side], (tag, space, q, i, float(u))
                assert trip_e[q, i, 0] == np.flatnonzero(pos[i] & (np.arange(B) != i))[side], (tag, space, q, i, float(u))


def test_a_row_with_one_item_of_positive_weight_gives_that_item():
    """B = 200, the default space: one negative sits opposite a tight cluster, so its row of D differs from every other row by about
    2 sqrt(B): 1 - M^2 / 4 clamps to 1e-8 and its log weight leads the others by more than 745, which underflow to exactly 0"""
    import recipe
    B, K = 200, 16
    e = np.zeros(K, np.float32)
    e[0] = 1.0
    x = e[None, :] + 0.01 * recipe.features(B, K, 3, "ddwsh_onehot")
    x[150] = -e
    lab = np.zeros((B, 2), np.float32)
    lab[:4, 0] = 1.0
    lab[4:, 1] = 1.0
    c = dict(x=x, y=x, lab=lab, beta=dw.case_beta(2))
    xs = tt(x)
    uni = np.stack([np.full((B, 2), u, np.float32) for u in (0.0, 0.5, LAST)])
    trip, w, _ = _mine([(xs, xs)] * 3, c, uni)
    for i in range(4):
        assert np.flatnonzero(w[0, i] > 0).tolist() == [150], (i, np.flatnonzero(w[0, i] > 0))
        assert trip[:, i, 1].tolist() == [150, 150, 150]
    assert np.array_equal(w[0], w[1]) and np.array_equal(w[0], w[2])


@pytest.mark.parametrize("tag", GOLDEN_TAGS)
def test_weights_against_the_restatement_and_the_references_q(golden, tag):
    g = golden("ddwsh.npz")
    c = _case(tag)
    B, K = c["x"].shape
    x, y = tt(c["x"]), tt(c["y"])
    uni = dw.case_uniforms(3, B, c["seed"])[:2]
    for space, modes in (("distances", ("intra", "cross")), ("embeddings", ("emb", None))):
        trip, w, dist = _mine([(x, x), (x, y)], c, uni, space)
        for q, mode in enumerate(modes):
            # (1) the float64 restatement on the kernel's own D
            M, dim = dw.mining_matrix(dist[q], K, space=space)
            want = _q(dw.sphere_weights(M, c["lab"], dim))
            _close(_q(w[q]), want, (tag, space, q, "q against the restatement on the kernel's D"))
            if mode is None:                                                         # the cross pair of the paper's space: the restatement alone
                continue
            # (2) the reference's recorded q: twice what the float64 restatement itself deviates on this CASE (the largest of its
            # three recorded distributions, tests/ddwshutil.py::Q_DEV; the mode's own figure is printed next to it)
            ref = g[f"{tag}_{mode}_q"].astype(np.float64)
            dev = float(np.abs(_q(w[q]) - ref).max())
            allowed = 2.0 * max(dw.Q_DEV[tag].values())
            print(f"{tag} {space} {mode}: max |q - reference q| {dev:.3e}, allowed {allowed:.3e} (the restatement's own on this mode: "
                  f"{dw.Q_DEV[tag][mode]:.3e})")
            assert dev <= allowed, (tag, space, mode, dev)
            # every negative the reference drew has positive weight here
            rt = g[f"{tag}_{mode}_trip"]
            for i in np.flatnonzero(rt[:, 1] >= 0):
                assert w[q, i, rt[i, 1]] > 0, (tag, mode, i)


def _edge(c, space="distances", grads=True):
    """sampler and loss of the step's three pairs against the restatement deciding on the kernel's own weights and distances"""
    B, K = c["x"].shape
    uni = dw.case_uniforms(3, B, 9, "edge")
    pairs = _three(c)
    trip, w, dist = _mine(pairs, c, uni, space)
    _check_sampler(c, trip, w, uni, c["tag"])
    exact = [dw.distances(a, b) for a, b in ((c["x"], c["x"]), (c["y"], c["y"]), (c["x"], c["y"]))]
    bound = (K + 16) * 2.0 ** -24                 # a K-term fmaf chain under a square root, on unit rows rounded twice; D <= 2
    for q in range(3):
        assert np.abs(dist[q] - exact[q]).max() <= bound, (c["tag"], q, np.abs(dist[q] - exact[q]).max(), bound)
    M, dim = dw.mining_matrix(dist[2], K, space=space)
    _close(_q(w[2]), _q(dw.sphere_weights(M, c["lab"], dim)), (c["tag"], space, "q"))
    loss, count, g, dbeta, dist2 = _loss(pairs, c, trip)
    assert np.array_equal(dist2, dist)
    want = [dw.margin_loss(a, b, c["lab"], c["beta"], trip[q], D=dist[q])
            for q, (a, b) in enumerate(((c["x"], c["x"]), (c["y"], c["y"]), (c["x"], c["y"])))]
    assert count.tolist() == [r["count"] for r in want]
    _close(loss, np.array([r["loss"] for r in want]), (c["tag"], "loss"))
    if grads and any(r["count"] for r in want):
        assert g[0][1] is None and g[1][1] is None and g[2][1] is not None
        _close(g[0][0], 2.0 * (want[0]["dx"] + want[0]["dy"]), (c["tag"], "d x, intra"))
        _close(g[1][0], 2.0 * (want[1]["dx"] + want[1]["dy"]), (c["tag"], "d y, intra"))
        _close(g[2][0], 2.0 * want[2]["dx"], (c["tag"], "d x, cross"))
        _close(g[2][1], 2.0 * want[2]["dy"], (c["tag"], "d y, cross"))
        _close(dbeta, 2.0 * sum(r["dbeta"] for r in want), (c["tag"], "d beta"))
    return trip, count


def test_edge_one_row_has_no_anchor():
    c = dw.edge_case(1, 8, 3, 1, p=0.9)
    trip, count = _edge(c)
    assert (trip == -1).all() and count.tolist() == [0, 0, 0]


def test_edge_two_rows():
    c = dw.edge_case(2, 8, 3, 2)
    c["lab"][:] = 0.0
    c["lab"][:, 1] = 1.0                                                             # both share a label: each shares with every item
    trip, _ = _edge(c)
    assert (trip == -1).all()


@pytest.mark.parametrize("space", dw.SPACES)
def test_edge_one_code_column(space):
    _edge(dw.edge_case(37, 1, 6, 3, p=0.25), space)                                  # unit rows are +-1: distances 1e-8 or 2


@pytest.mark.parametrize("space", dw.SPACES)
def test_edge_two_rounds_of_anchors_and_two_label_words(space):
    trip, count = _edge(dw.edge_case(257, 24, 80, 4, p=0.02), space)
    assert (trip[:, :, 0] >= 0).sum() > 300 and count.min() > 0


def test_edge_the_limits_once():
    trip, count = _edge(dw.edge_case(1024, 128, 80, 5, p=0.015))
    assert (trip[:, :, 0] >= 0).sum() > 1500 and count.min() > 0


def test_three_pairs_in_one_call_are_three_single_calls_and_repeat_bit_for_bit():
    c = dw.edge_case(130, 65, 70, 6, p=0.03)
    B = 130
    uni = dw.case_uniforms(3, B, 6, "bits")
    pairs = _three(c)
    before = [t.clone() for pr in pairs for t in pr]
    trip, w, dist = _mine(pairs, c, uni)
    trip2, w2, dist2 = _mine(pairs, c, uni)
    assert np.array_equal(trip, trip2) and np.array_equal(w, w2) and np.array_equal(dist, dist2)
    loss, count, g, dbeta, _ = _loss(pairs, c, trip)
    loss2, count2, g2, dbeta2, _ = _loss(pairs, c, trip)
    assert np.array_equal(loss, loss2) and np.array_equal(count, count2) and torch.equal(dbeta, dbeta2) and count.min() > 0
    one_dbeta = []
    for q, pr in enumerate(pairs):
        t1, w1, d1 = _mine([pr], c, uni[q:q + 1])
        assert np.array_equal(t1[0], trip[q]) and np.array_equal(w1[0], w[q]) and np.array_equal(d1[0], dist[q])
        l1, c1, g1, db1, _ = _loss([pr], c, trip[q:q + 1])
        assert l1[0] == loss[q] and c1[0] == count[q]
        one_dbeta.append(db1)
        for a, b, a2 in zip(g[q], g1[0], g2[q]):
            assert (a is None and b is None) or (torch.equal(a, b) and torch.equal(a, a2) and bool(a.any()))
    assert g[0][1] is None and g[1][1] is None and g[2][1] is not None              # an intra-modal pair gives dv = None
    _close(dbeta, num(one_dbeta[0] + one_dbeta[1] + one_dbeta[2]).astype(np.float64), "d beta over the pairs")
    assert all(torch.equal(t, b) for t, b in zip([t for pr in pairs for t in pr], before))


def test_refusals_name_their_entry():
    import cmh_native as N
    from train.DDWSH.loss import MarginLoss
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(N.NativeError, match=r"dws_distances.*128"):
        MarginLoss(2).to(DEV)(z(4, 129), z(4, 129), z(4, 2))
    with pytest.raises(N.NativeError, match=r"dws_distances.*1024"):
        MarginLoss(2).to(DEV)(z(1025, 16), z(1025, 16), z(1025, 2))
    with pytest.raises(N.NativeError, match="dws_mine.*1024"):
        N.dws_mine(z(1, 4, 4), z(4, 1025), 8, z(1, 4, 2))
    with pytest.raises(N.NativeError, match="dws_margin_loss"):
        N.dws_margin_loss([(z(4, 8), z(4, 8))], z(4, 2), z(3), torch.zeros(1, 4, 2, dtype=torch.int32, device=DEV))     # beta of another length
    out = torch.full((64,), 7, dtype=torch.int32, device=DEV)
    lib = N.lib()
    ws = N.workspace(lib.cmh_dws_workspace_bytes(4, 8, 2), out.device, "loss")
    d, lab, uni = z(1, 4, 4), z(4, 2), z(1, 4, 2)
    assert lib.cmh_dws_mine(N.ptr(d), 1, N.ptr(lab), 4, 8, 2, 0.5, 2, N.ptr(uni), N.ptr(out), None, N.ptr(ws), ws.numel(), None) == -1
    assert b"dws_mine: space=2" in lib.cmh_last_error()
    assert lib.cmh_dws_mine(N.ptr(d), 1, N.ptr(lab), 4, 8, 2, 0.5, 0, N.ptr(uni), N.ptr(out), None, N.ptr(ws), 8, None) == -1
    assert b"dws_mine: workspace too small" in lib.cmh_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                                    # nothing was launched


def test_triplets_handed_in_out_of_range_skip_their_anchor():
    c = _case("B12_K16_C4")
    x = tt(c["x"])
    trip = np.full((1, 12, 2), -1, np.int32)
    trip[0, 3] = (12, 0)
    trip[0, 4] = (0, -5)
    loss, count, grads, dbeta, _ = _loss([(x, x)], c, trip)
    assert loss[0] == 0.0 and count[0] == 0 and not grads[0][0].any() and not dbeta.any()


def _trainer(tmp_path, monkeypatch, *extra):
    import argparse
    import sys
    import recipe
    import main
    import dataset.synthetic as dsy
    ck = tmp_path / "clip.pt"
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, ck)
    monkeypatch.setattr(dsy, "SOT", 510)
    monkeypatch.setattr(dsy, "EOT", 511)
    monkeypatch.setattr(sys, "argv", ["main.py", "-clip-path", str(ck), "--save-dir", str(tmp_path / "run"), "--batch-size", "16", "--num-workers", "0",
                                      "--resolution", "64", "--max-words", "16", "--query-num", "24", "--train-num", "32",
                                      "--synthetic-size", "120", *extra])
    torch.manual_seed(3)
    return main.trainers["DWSH"](argparse.Namespace(method="DWSH", dataset="synthetic", output_dim=16, is_train=True), 0), ck


def test_two_epochs_checkpoint_loads_as_dsph_and_serves_queries(tmp_path, monkeypatch):
    """Registry -> DDWSHTrainer -> two epochs on the synthetic set with the tiny towers; the checkpoint has DSPH's keys (no beta) and
    gives equal codes through QueryEncoder as DWSH and as DSPH"""
    from query import QueryEncoder
    tr, ck = _trainer(tmp_path, monkeypatch, "--epochs", "2")
    assert type(tr).__name__ == "DDWSHTrainer" and type(tr.model).__name__ == "MDDWSH" and tr.global_step == 4
    assert len(tr.optimizer.param_groups) == 4 and tr.optimizer.param_groups[3]["params"][0] is tr.criterion.beta
    assert tr.criterion.beta.shape == (tr.args.nclass,) and tr.criterion.beta.is_cuda
    assert not torch.equal(tr.criterion.beta.detach(), torch.full_like(tr.criterion.beta, 1.2))       # beta moved
    model_file = tmp_path / "run" / "DWSH" / "synthetic" / "16" / "model-1.pth"
    assert model_file.exists()
    state = torch.load(model_file, map_location="cpu")
    from model.DSPH import MDSPH
    dsph = MDSPH(outputDim=16, clipPath=str(ck), saveDir=str(tmp_path / "log"))
    assert set(state) == set(dsph.state_dict()) and not any("beta" in k for k in state)
    assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters()) and bool(torch.isfinite(tr.criterion.beta).all())
    q_img, q_txt, _ = tr.get_code(tr.query_loader, tr.args.query_num)
    assert set(q_img.unique().tolist()) <= {-1.0, 0.0, 1.0}
    encs = [QueryEncoder(method, str(model_file), str(ck), 16, max_words=16, resolution=64) for method in ("DWSH", "DSPH")]
    for batch in tr.query_loader:
        image, text = batch[0].to(DEV), batch[1]
        with torch.no_grad():
            got_i = [enc.rule(enc.model.encode_image(image)) for enc in encs]
        got_t = [enc.encode_tokens(text) for enc in encs]
        assert torch.equal(got_i[0], got_i[1]) and torch.equal(got_t[0], got_t[1])     # one checkpoint under both names: equal codes
        assert set(got_i[0].unique().tolist()) <= {-1.0, 0.0, 1.0} and got_i[0].shape == (image.shape[0], 16)


def test_equal_seeds_give_equal_losses(tmp_path, monkeypatch):
    losses = []
    for run, seed in enumerate(("5", "5", "6")):
        (tmp_path / f"r{run}").mkdir()
        tr, _ = _trainer(tmp_path / f"r{run}", monkeypatch, "--epochs", "0", "--dws-seed", seed)
        assert tr.criterion.seed == int(seed)
        tr.change_state(mode="train")
        for grp in tr.optimizer.param_groups:
            grp["t_total"] = 4
        torch.manual_seed(11)
        losses.append([float(tr._step(image, text, label)) for image, text, label, index in list(tr.train_loader)[:2]])
    print(f"losses per seed: {losses}")
    assert losses[0] == losses[1] and all(np.isfinite(v) for run in losses for v in run)
    assert losses[0] != losses[2]                                                     # another seed draws other triplets


def test_ddwsh_training_trajectory_matches_reference(golden):
    """Three steps of the DDWSH loop (tape forward -> LinearHash heads -> the three-pair margin loss on the reference's triplets ->
    backward through heads and towers -> fused BertAdam over FOUR groups) on the tiny CLIP: the loss of every step, the final parameters
    and the final beta against the REFERENCE's own run on the CPU (tests/golden/make_golden23.py; the heads in eval mode on both sides)"""
    from types import SimpleNamespace
    import ddbhutil as dd
    import dchmtutil as du
    import mschutil as ms
    from model.base.optimization import BertAdam
    from model.modelbase import LinearHash
    from test_gpu_clip import _clip
    from train.DDWSH.hash_train import DDWSHTrainer
    from train.DDWSH.loss import MarginLoss
    g = golden("ddwsh_traj.npz")
    assert float(g["gap_over_err"]) >= 100.0
    clip = _clip(du.CFG, du.SEED, "f32")
    ih, th = LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval(), LinearHash(du.CFG["embed_dim"], dd.TRAJ_K).eval()
    dd.fill_linear_head(ih, 1)
    dd.fill_linear_head(th, 2)
    ih, th = ih.to(DEV), th.to(DEV)
    crit = MarginLoss(du.C).to(DEV)
    crit.beta.data.copy_(tt(dw.traj_beta(du.C)))
    opt = BertAdam([{"params": [p for _, p in clip.named_parameters()], "lr": du.CLIP_LR}, {"params": ih.parameters(), "lr": du.OPT["lr"]},
                    {"params": th.parameters(), "lr": du.OPT["lr"]}, {"params": crit.parameters(), "lr": du.OPT["lr"]}], **du.OPT)
    me = SimpleNamespace(criterion=crit)
    losses = []
    for step in range(dd.TRAJ_STEPS):
        img, txt, lab = dd.traj_batch(step)
        loss = DDWSHTrainer.compute_loss(me, ih(clip.encode_image(img.to(DEV))), th(clip.encode_text(txt.to(DEV))), lab.to(DEV).float(),
                                         ti(g["trips"][step]))
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"DDWSH trajectory: losses {losses} (reference {g['losses'].tolist()})")
    np.testing.assert_allclose(np.array(losses), g["losses"], rtol=1e-4)
    named = dict(clip.named_parameters())
    named.update({"image_hash." + n: p for n, p in ih.named_parameters()})
    named.update({"text_hash." + n: p for n, p in th.named_parameters()})
    worst = 0.0
    for key in g.files:
        if not key.startswith("p_"):
            continue
        ref = g[key]
        err = np.abs(ms.cut(named[key[2:]].detach().cpu().numpy()) - ref).max() / max(np.abs(ref).max(), 1e-6)
        worst = max(worst, err)
        assert err < 1e-4, (key, err)
    err = np.abs(num(crit.beta) - g["beta"]).max() / np.abs(g["beta"]).max()
    print(f"DDWSH trajectory: worst parameter error {worst:.2e} of max, beta {err:.2e}")
    assert err < 1e-4 and np.abs(g["beta"] - dw.traj_beta(du.C)).max() > 1e-4         # ... and the reference's beta moved
