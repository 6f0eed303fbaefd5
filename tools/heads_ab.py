"""Every head and loss entry point of csrc/heads.hip, heads2.hip, heads_bwd.hip, losses.hip, msl.hip, qmi.hip and mith.hip, once per case, on
seeded inputs: the check behind a change of their host code or shared helpers (csrc/head_common.h), which must leave every output bit and
every launch as they were.

    python tools/heads_ab.py run OUT.json                        one library (CMH_LIB picks it), a fresh process each
    python tools/heads_ab.py compare A.json B.json [A2.json]     per-entry-point verdict; exit status 1 on any difference
                                                                  (A2: a second run of A - what it does not reproduce is named, not compared)
    python tools/heads_ab.py launches TRACE_DIR_A TRACE_DIR_B     the ordered (kernel, grid, workgroup) lists of two
                                                                  `rocprofv3 --kernel-trace --output-format csv -d DIR -- ... run` runs, kernel
                                                                  names without their arguments and after RENAMED; exit status 1 if they differ

`run` records the sha256 of every output's bytes and synchronises the device between calls.  Calls go through the wrappers the trainers use
(cmh_native, backward_ops, mith_ops, mith_train_ops and the loss modules under train/); cases and inputs are the edge shapes of
tests/lossutil.py and tests/mithedgeutil.py, plus: DCHMT with cosine similarity and an all-zero image matrix (the any-non-zero flag selects
the raw rows), the LinearHash forward with the pair softmax and both code kernels, TwDH's targets / loss / backward, and - in a child
process with CMH_BAYES_MFMA=0, which the library reads once - the InfoNCE and Bayesian entries on their butterfly kernels.

The DSPH, DCHMT, DNPH, TwDH, sq-diff, Bayesian and InfoNCE forwards finish through f64 atomics, so `compare` takes a second run of A as the
control: an array A does not reproduce is named instead of compared, and must be a scalar loss of one of those entries."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)

ATOMIC_LOSSES = ("hyp/", "dchmt/", "dchmt_zero_image/", "dnph/", "twdh/", "sqdiff/", "bayes/", "nce/", "mfma0/bayes/", "mfma0/nce/")
RENAMED = {"row_normalize_kernel": "normalize_rows_kernel", "hyp_normalize_kernel": "normalize_rows_kernel",
           "plain_normalize_kernel": "normalize_rows_kernel", "qmi_norms_kernel": "row_norms2_kernel", "spl_norms_kernel": "row_norms2_kernel"}


def run(out_path, mfma0=False):
    import numpy as np
    import torch
    import cmh_native as N
    import lossutil as L
    import mithedgeutil as U
    from mith_train_ops import BayesianLossFn, InfoNceFn

    dev = "cuda:0"
    digests = {}

    def keep(key, t):
        torch.cuda.synchronize()
        a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
        assert key not in digests, key
        digests[key] = f"{hashlib.sha256(a.tobytes()).hexdigest()} {a.dtype} {list(a.shape)}"

    def on(t):
        return t.detach().clone().to(dev).requires_grad_(True)

    def grads(key, loss, up, leaves, names):
        keep(f"{key}/loss", loss)
        (up * loss).backward()
        for n, l in zip(names, leaves):
            keep(f"{key}/{n}", l.grad)

    def mith_losses(prefix):
        for case in U.BAYES_CASES:
            c = U.bayes_case(*case)
            x = on(c["batch"])
            grads(f"{prefix}bayes/{case}", BayesianLossFn.apply(c["bank"].to(dev), x, c["bank_label"].to(dev), c["label"].to(dev)),
                  U.UPSTREAM["bayes"], [x], ["dbatch"])
        for case in U.NCE_CASES:
            c = U.nce_case(*case)
            a, b = on(c["a"]), on(c["b"])
            grads(f"{prefix}nce/{case}", InfoNceFn.apply(a, b, case[1], U.NCE_TEMPERATURE), U.UPSTREAM["nce"], [a, b], ["da", "db"])

    if mfma0:
        assert os.environ.get("CMH_BAYES_MFMA") == "0"
        mith_losses("mfma0/")
    else:
        import mith_ops as M
        from backward_ops import BatchNorm1dTrain, DchmtLoss, DnphLoss, HypLoss, LinearAct, TwdhLoss
        from mith_train_ops import AddPosFn, BitHashFn, GeluFn, L2NormFn, LtaFn, SqDiffSumFn
        from train.DHaPH.MSLoss import MSLoss
        from train.DMsH_LN.MSLOSS import MultiSimilarityLoss
        from train.DNpH_TMM.loss import qmi_loss

        # ---- csrc/losses.hip, heads_bwd.hip, heads2.hip, qmi.hip, msl.hip (spl): the cases of tests/test_gpu_loss_edges.py
        for case in L.HYP_CASES:
            c, _, tensors, names = L.problem("hyp", case)
            lv = [on(t) for t in tensors]
            grads(f"hyp/{case}", HypLoss.apply(lv[0], lv[1], c["lab"].to(dev), lv[2], c["thr"], c["alpha"]), L.UPSTREAM["hyp"], lv, names)
        for case in L.DCHMT_CASES:
            c, _, tensors, names = L.problem("dchmt", case)
            lv = [on(t) for t in tensors]
            grads(f"dchmt/{case}", DchmtLoss.apply(lv[0], lv[1], c["lab"].to(dev), *c["cfg"]), L.UPSTREAM["dchmt"], lv, names)
        g = L.gen(31, 5, 8, 3)                                            # anynz == 0: the raw (zero) image rows are selected
        txt, lab = L.sign_rows(5, 8, g), L.labels(5, 3, 0.4, g)
        for loss_type in ("l1", "l2"):
            keep(f"dchmt_zero_image/{loss_type}/loss", N.dchmt_loss(torch.zeros(5, 8, device=dev), txt.to(dev), lab.to(dev), 8, "cosine", loss_type, 0.5, 0.1))
        for case in L.DNPH_CASES:
            c, _, tensors, names = L.problem("dnph", case)
            lv = [on(t) for t in tensors]
            ni, nt = (None if c[k] is None else c[k].to(dev) for k in ("noise_i", "noise_t"))
            lab = c["lab"].to(dev)
            grads(f"dnph/{case}", DnphLoss.apply(lv[0], lv[1], lv[2], lv[3], lab, lv[4], ni, nt, 1.0, 0.1), L.UPSTREAM["dnph"], lv, names)
            for n, v in zip(("total", "loss1", "noise"), N.dnph_loss(*(l.detach() for l in lv[:4]), lab, lv[4].detach(), ni, nt, 1.0, 0.1)):
                keep(f"dnph/{case}/forward/{n}", v)
        for case in L.QMI_CASES:
            c, _, tensors, names = L.problem("qmi", case)
            lv = [on(t) for t in tensors]
            grads(f"qmi/{case}", qmi_loss(images=lv[0], texts=lv[1], targets=c["lab"].to(dev)), L.UPSTREAM["qmi"], lv, names)
        for case in L.SPL_CASES:
            for variant in ("same", "cross"):
                c, _, tensors, names = L.problem("spl", case, variant)
                lv = [on(t) for t in tensors]
                crit = MSLoss(temperature=L.SPL_TEMPERATURE, totalepoch=12, self_paced=True)
                grads(f"spl/{case}/{variant}", crit(lv[0], lv[-1], c["lab"].to(dev), int(case[3] * 4)), L.UPSTREAM["spl"], lv, names)
        for M_, N_, K_ in L.LINEAR_SHAPES:
            for act in (0, 1, 2):
                for use_mask in (False, True):
                    c = L.linear_case(M_, N_, K_, act, use_mask)
                    key = f"linear/{(M_, N_, K_)}/act{act}/mask{int(use_mask)}"
                    mask, dy = None if c["mask"] is None else c["mask"].to(dev), c["dy"].to(dev)
                    lv = [on(c[k]) for k in ("x", "w", "b")]
                    if K_ % 4 == 0:
                        y = LinearAct.apply(lv[0], lv[1], lv[2], act, mask, L.LINEAR_DROP)
                        keep(f"{key}/y", y)
                        y.backward(dy)
                        got = [l.grad for l in lv]
                    else:                                               # the forward refuses this K: the backward entry itself
                        x, w = lv[0].detach(), lv[1].detach()
                        y = L.linear_act(c["x"].double(), c["w"].double(), c["b"].double(), act, c["mask"], L.LINEAR_DROP).float().to(dev)
                        got = [torch.empty_like(x), torch.empty_like(w), torch.empty(N_, dtype=torch.float32, device=dev)]
                        ws = N.workspace(M_ * N_ * 4 + 256, x.device, "bwd")
                        N.check(N.lib().cmh_linear_act_backward(N.ptr(x), N.ptr(w), N.ptr(y), N.ptr(dy), N.ptr(mask), 1.0 / (1.0 - L.LINEAR_DROP), act,
                                                                N.ptr(got[0]), N.ptr(got[1]), N.ptr(got[2]), M_, N_, K_, N.ptr(ws), ws.numel(),
                                                                N.stream_ptr(x.device)), "cmh_linear_act_backward")
                    for n, t in zip(("dx", "dW", "db"), got):
                        keep(f"{key}/{n}", t)
        c = L.linear_case(67, 5, 260, 1, True)                            # forward + the code kernels
        y = N.linear_act(c["x"].to(dev), c["w"].to(dev), c["b"].to(dev), N.ACT_TANH, c["mask"].to(dev), L.LINEAR_DROP)
        p = N.pair_softmax(y[:, :4].contiguous())
        keep("codes/linear_act", y), keep("codes/pair_softmax", p), keep("codes/sign_codes", N.sign_codes(y))
        keep("codes/pair_argmax_codes", N.pair_argmax_codes(p))
        for B, d in L.BATCHNORM_SHAPES:
            c = L.batchnorm_case(B, d)
            lv = [on(c[k]) for k in ("x", "w", "b")]
            y = BatchNorm1dTrain.apply(lv[0], lv[1], lv[2], L.BATCHNORM_EPS)
            keep(f"batchnorm/{(B, d)}/y", y)
            y.backward(c["dy"].to(dev))
            rm, rv = c["rm"].to(dev), c["rv"].to(dev)
            N.check(N.lib().cmh_batchnorm1d_update_running(N.ptr(lv[0].detach()), L.BATCHNORM_MOMENTUM, N.ptr(rm), N.ptr(rv), B, d,
                                                           N.stream_ptr(rm.device)), "cmh_batchnorm1d_update_running")
            for n, t in zip(("running_mean", "running_var", "dx", "dw", "db"), [rm, rv] + [l.grad for l in lv]):
                keep(f"batchnorm/{(B, d)}/{n}", t)
        B, K, Cn = 33, 65, 7                                              # TwDH
        g = L.gen(32, B, K)
        lab = L.labels(B, Cn, 0.3, g)
        center, rc = torch.sign(torch.randn(Cn, K, generator=g)), torch.sign(torch.randn(K, generator=g))
        center[:2, ::3] = 0                                               # some means are exactly zero: random_center decides
        code = N.twdh_targets(lab.to(dev), center.to(dev), rc.to(dev))
        keep("twdh/targets", code)
        pi, pt = (N.pair_softmax(torch.randn(B, 2 * K, generator=g).to(dev)).requires_grad_(True) for _ in range(2))
        nce, quan = TwdhLoss.apply(pi, pt, code)
        keep("twdh/nce", nce), keep("twdh/quan", quan)
        (1.7 * nce + 0.3 * quan).backward()
        keep("twdh/backward/dp_img", pi.grad), keep("twdh/backward/dp_txt", pt.grad)

        # ---- csrc/mith.hip and the multi-similarity loss of msl.hip: the cases of tests/test_gpu_mith_edges.py
        for case in U.LTA_CASES:
            c = U.lta_case(*case)
            l0, L_, top_k = c["geom"]
            tokens, kpm = on(c["tokens"]), None if c["kpm"] is None else c["kpm"].to(dev)
            out = LtaFn.apply(tokens, c["sim"].to(dev), kpm, l0, L_, top_k)
            keep(f"lta/{case}/merge", out), keep(f"lta/{case}/forward", M.lta(tokens.detach(), c["sim"].to(dev), kpm, l0, L_, top_k))
            out.backward(U.UPSTREAM["lta"] * c["dmerge"].to(dev))
            keep(f"lta/{case}/dtokens", tokens.grad)
        for case in U.BITHASH_CASES:
            c = U.bithash_case(*case)
            lv = [on(c[k]) for k in ("x", "w", "b")]
            y = BitHashFn.apply(*lv)
            keep(f"bithash/{case}/y", y)
            y.backward(U.UPSTREAM["bithash"] * c["dy"].to(dev))
            for n, l in zip(("dx", "dw", "db"), lv):
                keep(f"bithash/{case}/{n}", l.grad)
        for case in U.L2NORM_CASES:
            c = U.l2norm_case(*case)
            x = on(c["x"])
            y = L2NormFn.apply(x)
            keep(f"l2norm/{case}/y", y)
            y.backward(U.UPSTREAM["l2norm"] * c["dy"].to(dev))
            keep(f"l2norm/{case}/dx", x.grad)
        c = U.mix_case()
        for n, t in zip(("B", "H_img", "H_txt"), M.mith_mix(*(c[k].to(dev) for k in ("ic", "it", "tc", "tt")), U.MIX_LAMBDA)):
            keep(f"mix/{n}", t)
        g = U.gen(21, 3, 5, 7)
        x, pe, dy = (torch.randn(*s, generator=g) for s in ((3, 5, 7), (9, 7), (3, 5, 7)))
        leaf = on(x)
        y = AddPosFn.apply(leaf, pe.to(dev))
        keep("addpos/y", y)
        y.backward(dy.to(dev))
        keep("addpos/dx", leaf.grad)
        c = U.gelu_case()
        leaf = on(c["x"])
        y = GeluFn.apply(leaf)
        keep("gelu/y", y)
        y.backward(c["dy"].to(dev))
        keep("gelu/dx", leaf.grad)
        for n in U.SQDIFF_SIZES:
            c = U.sqdiff_case(n)
            a, b = on(c["a"]), on(c["b"])
            grads(f"sqdiff/{n}", SqDiffSumFn.apply(a, b), U.UPSTREAM["sqdiff"], [a, b], ["da", "db"])
        mith_losses("")
        for case in U.MSL_CASES:
            for cross in (False, True):
                c, _, tensors, names = U.msl_problem(case, cross)
                lv = [on(t) for t in tensors]
                loss = MultiSimilarityLoss()(lv[0], c["code"].to(dev), feat2=lv[1] if cross else None)
                grads(f"msl/{case}/{'cross' if cross else 'self'}", loss, U.UPSTREAM["msl"], lv, names)
        torch.cuda.synchronize()

        # the butterfly forms of the InfoNCE / Bayesian entries: the switch is read once per process, so a process of their own
        child = out_path + ".mfma0"
        subprocess.run([sys.executable, os.path.abspath(__file__), "run-mfma0", child], env=dict(os.environ, CMH_BAYES_MFMA="0"), check=True)
        more = json.load(open(child))["outputs"]
        assert not set(more) & set(digests)
        digests.update(more)
        os.remove(child)
    with open(out_path, "w") as f:
        json.dump({"lib": N.LIB_PATH, "outputs": digests}, f, indent=0)
    print(f"{len(digests)} outputs of {N.LIB_PATH} -> {out_path}")


def compare(pa, pb, pa2=None):
    a, b = json.load(open(pa)), json.load(open(pb))
    print(f"A = {a['lib']}\nB = {b['lib']}")
    keys = sorted(set(a["outputs"]) | set(b["outputs"]))
    bad = {k for k in keys if a["outputs"].get(k) != b["outputs"].get(k)}
    loose = {k for k in keys if a["outputs"].get(k) != json.load(open(pa2))["outputs"].get(k)} if pa2 else set()
    for k in loose:      # what a library does not reproduce against itself: one f64-atomic scalar loss, never a tensor
        assert k.startswith(ATOMIC_LOSSES) and a["outputs"][k].endswith((" []", " [1]")), f"{k} is not reproducible by A itself: {a['outputs'][k]}"
    entry = {}
    for k in keys:       # an entry-point call = the key up to the array's own name
        entry.setdefault(k.rsplit("/", 1)[0], []).append(k)
    for e, ks in entry.items():
        word = "DIFFERENT" if any(k in bad - loose for k in ks) else "identical"
        n_loose = sum(k in loose for k in ks)
        print(f"{word}  {e}  ({len(ks)} arrays" + (f", {n_loose} not reproducible by A itself" if n_loose else "") + ")")
    print(f"{len(keys)} arrays, {len(entry)} entry-point calls: {len(bad - loose)} reproducible arrays differ; "
          f"{len(loose)} scalar losses differ between two runs of A ({sorted(loose)}), {len(bad & loose)} of them between A and B")
    return 1 if bad - loose else 0


def launches(dir_a, dir_b):
    from entry_points_ab import launch_lists

    def plain(name):     # "cmh::(anonymous namespace)::hyp_normalize_kernel(float const*, ...)" -> "normalize_rows_kernel"
        base = name.split("(anonymous namespace)::")[-1].split("(")[0].split("cmh::")[-1]
        return RENAMED.get(base, base)
    got = [[[[plain(n), g, w] for n, g, w in l] for l in launch_lists(d)] for d in (dir_a, dir_b)]
    print("kernel names compared without their arguments, after " + ", ".join(f"{k} -> {v}" for k, v in RENAMED.items()))
    for d, lists in zip((dir_a, dir_b), got):
        print(f"{d}: {[len(l) for l in lists]} launches per stream, sha256 {hashlib.sha256(json.dumps(lists).encode()).hexdigest()}")
    if got[0] == got[1]:
        print("the ordered (kernel, grid, workgroup) lists are equal")
        return 0
    for la, lb in zip(*got):
        for i, (x, y) in enumerate(zip(la, lb)):
            if x != y:
                print(f"first difference at launch {i}:\n  {x}\n  {y}")
                return 1
    print("the lists differ in length")
    return 1


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd in ("run", "run-mfma0"):
        run(sys.argv[2], mfma0=cmd == "run-mfma0")
    elif cmd == "compare":
        sys.exit(compare(*sys.argv[2:5]))
    elif cmd == "launches":
        sys.exit(launches(*sys.argv[2:4]))
    else:
        sys.exit(__doc__)
