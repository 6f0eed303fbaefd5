"""Flags of the training-free fit (no upstream counterpart)."""
from argsbase import method_args

FLAGS = [("--projection", str, "pca", "pca: the leading eigenvectors of the pooled covariance; random: Gaussian, drawn from --seed"),
         ("--rotation", str, "itq", "itq: iterative quantisation from the identity; none: no rotation (pca: PCAH, random: LSH)"),
         ("--itq-iters", int, 50, "ITQ iterations"),
         ("--fit-num", int, 0, "training items the fit reads, in loader order; 0: all of them")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
