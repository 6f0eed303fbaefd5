"""Do soft queries rank better than binary ones?  DSPH is trained on the learnable synthetic set (dataset/synthetic.py with signal:
class patterns in the images, class tokens in the captions) for a few epochs at 16, 32 and 64 bit on a tiny CLIP; the database side
is indexed (utils.retrieval.CodeIndex) and the query side asks it twice, image -> text and text -> image:
  binary   CodeIndex.search(sign codes, k)           Hamming distance, ties by database index
  soft     CodeIndex.search_soft(head outputs, k)    the weighted distance of csrc/retrieval_soft.hip, ties by database index
Per (bits, direction, kind): P@10, mAP@50 (AP@50 = the mean of the precisions at the relevant positions among the first 50, 0 when
there is none; relevance = a shared label, labels gathered from idx on the host) and the mean size of the tie group at the 10th
place (database items at exactly the 10th neighbour's distance, counted inside the first min(N, 4096) results); and over the WHOLE
database, by counting, the project's headline metric: mAP = CodeIndex.map (binary) / CodeIndex.map_soft (soft), both with ties by
database index, and for the soft ranking the mean per-query ROC-AUC (auc_from_rank_sum).  ONE JSON line.

    python tools/soft_quality.py [--epochs 6] [--bits 16 32 64] [--out FILE]

The synthetic set is small and its text codes are near-degenerate; the numbers describe this set, nothing else."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "clip-based-cross-modal-hashing_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def metrics(idx, dist, qL, rL):
    """idx / dist [Q, k] on any device, labels f32 [Q, C] / [N, C] -> dict of P@10, mAP@50, tie10."""
    import torch
    idx, dist = idx.cpu().long(), dist.cpu()
    rel = (torch.einsum("qc,qkc->qk", qL, rL[idx]) > 0).double()
    p10 = rel[:, :10].mean(1)
    top = rel[:, :50]
    prec = top.cumsum(1) / torch.arange(1, top.shape[1] + 1, dtype=torch.float64)
    hits = top.sum(1)
    ap = torch.where(hits > 0, (prec * top).sum(1) / hits.clamp(min=1), torch.zeros_like(hits))
    tie = (dist == dist[:, 9:10]).sum(1).double()
    return {"P@10": round(float(p10.mean()), 4), "mAP@50": round(float(ap.mean()), 4), "tie10": round(float(tie.mean()), 2)}


def one(bits, args, clip_file):
    import torch

    import dataset.synthetic as ds
    import main
    from code_rules import sign_code
    from utils.retrieval import CodeIndex, auc_from_rank_sum
    ds.SOT, ds.EOT = 510, 511                                      # the tiny CLIP's vocabulary
    ds.SyntheticPairs.signal = 2.0
    run = tempfile.mkdtemp(prefix="cmh_soft_quality_")
    sys.argv = ["main.py", "-clip-path", clip_file, "--save-dir", run, "--batch-size", "32", "--num-workers", "0", "--resolution", "64",
                "--max-words", "16", "--query-num", str(args.queries), "--train-num", str(args.train), "--synthetic-size",
                str(args.size), "--epochs", "0", "--gemm-dtype", "f32", "--lr", "0.001", "--clip-lr", "0.0003"]
    torch.manual_seed(0)
    tr = main.trainers["DSPH"](argparse.Namespace(method="DSPH", dataset="synthetic", output_dim=bits, is_train=True), 0)
    for grp in tr.optimizer.param_groups:
        grp["t_total"] = args.epochs * len(tr.train_loader)
    for epoch in range(args.epochs):
        tr.train_epoch(epoch)
    tr.change_state(mode="valid")
    raw = lambda i, t, b: (tr.model.encode_image(i), tr.model.encode_text(t))      # the tanh heads' outputs, before sign()
    with torch.no_grad():
        q_img, q_txt, _ = tr._code_loop(tr.query_loader, tr.args.query_num, raw)
        r_img, r_txt, _ = tr._code_loop(tr.retrieval_loader, tr.args.retrieval_num, raw)
    qL, rL = tr.query_labels.float(), tr.retrieval_labels.float()
    k = min(r_img.shape[0], 4096)
    out = {"queries": q_img.shape[0], "database": r_img.shape[0], "k": k}
    for name, u, r in (("i2t", q_img, r_txt), ("t2i", q_txt, r_img)):
        index = CodeIndex(sign_code(r), rL)
        out[name] = {"distinct_database_codes": int(torch.unique(sign_code(r), dim=0).shape[0]),
                     "binary": metrics(*index.search(sign_code(u), k)[:2], qL, rL),
                     "soft": metrics(*index.search_soft(u, k)[:2], qL, rL)}
        mp, _, relevant, rank_sum = index.map_soft(u, qL, return_ap=True)
        out[name]["binary"]["mAP"] = round(float(index.map(sign_code(u), qL)), 4)
        out[name]["soft"]["mAP"] = round(float(mp), 4)
        out[name]["soft"]["AUC"] = round(float(torch.nanmean(auc_from_rank_sum(rank_sum, relevant, index.size))), 4)
    return out


def main_():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bits", type=int, nargs="*", default=[16, 32, 64])
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--size", type=int, default=2600, help="items of the synthetic set")
    ap.add_argument("--queries", type=int, default=500)
    ap.add_argument("--train", type=int, default=800)
    ap.add_argument("--out", default="", help="append the JSON line to this file")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("soft_quality needs a GPU: the model trains and the index is searched there")
    import recipe
    clip_file = os.path.join(tempfile.mkdtemp(prefix="cmh_soft_quality_"), "clip.pt")
    torch.save({k: torch.from_numpy(v) for k, v in recipe.clip_state_dict(recipe.CLIP_TINY, 7).items()}, clip_file)
    line = {"tool": "soft_quality", "method": "DSPH", "epochs": args.epochs, "bits": {}}
    for bits in args.bits:
        line["bits"][str(bits)] = one(bits, args, clip_file)
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main_()
