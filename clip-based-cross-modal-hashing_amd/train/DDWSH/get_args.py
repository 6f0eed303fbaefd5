"""DDWSH flags.  Margin, beta and the lower cutoff are the reference's (train/DDWSH/get_args.py: margin 0.2, beta 1.2;
train/DDWSH/loss.py:85: lower_cutoff 0.5).  --dws-space picks what the miner measures: `distances` is what the reference runs (it hands
the miner the distance matrix as its batch, loss.py:22), `embeddings` is the form of Wu et al. (ICCV 2017).  --similarity-function is
the reference's own flag, which its trainer never reads: accepted and ignored.  The reference's save_dir reads the undefined
`args.loss` and `args.miner`; here it follows the other methods (<save-dir>/DWSH/<dataset>/<bits>)."""
from argsbase import method_args

SPACES = ("distances", "embeddings")
FLAGS = [("--dws-margin", float, 0.2, "margin m of relu(D_ap - beta + m) and relu(beta - D_an + m)"),
         ("--dws-beta", float, 1.2, "initial value of the per-class boundaries beta [C]"),
         ("--dws-cutoff", float, 0.5, "the mining distances are clamped from below to this before they are weighted"),
         ("--dws-space", str, "distances", "distances: mine on the rows of the distance matrix, dim = B (upstream); "
                                           "embeddings: on the distances themselves, dim = K (the paper)"),
         ("--dws-seed", int, 0, "seed of the sampler's uniforms: equal seeds give equal runs"),
         ("--similarity-function", str, "euclidean", "upstream's flag; not read")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
