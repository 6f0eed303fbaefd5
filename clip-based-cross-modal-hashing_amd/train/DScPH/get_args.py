"""DScPH flags.  The six CPF scalars are the reference's constants (train/DScPH/CPF_loss.py:17-22), the quantisation weight is the 1 of
its step (train/DScPH/hash_train.py:70); --hypseed and --alpha are the reference's own flags (train/DScPH/get_args.py:11-12), which its
trainer never reads: accepted and ignored."""
from argsbase import method_args

FLAGS = [("--cpf-tau", float, 0.9, "a negative class adds to the loss only where its cosine is above tau"),
         ("--cpf-psi", float, 0.7, "offset of the negative term: (c - psi) exp((c - mu) sn)"),
         ("--cpf-sp", float, 1.3, "scale inside the positive term's exponential"),
         ("--cpf-sn", float, 1.3, "scale inside the negative term's exponential"),
         ("--cpf-mu", float, 1.0, "centre of the negative term's exponential"),
         ("--cpf-b", float, 2.0, "constant added to the true-positive mass tp"),
         ("--quant-weight", float, 1.0, "factor on the two quantisation terms mean(sigma(z) (1 - sigma(z)))"),
         ("--hypseed", int, 0, "upstream's flag; not read"),
         ("--alpha", float, 0.8, "upstream's flag; not read")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
