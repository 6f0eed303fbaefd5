"""Flags of the training-free fit (no upstream counterpart)."""
from argsbase import method_args

FLAGS = [("--projection", str, "pca", "pca: the leading eigenvectors of the pooled covariance; random: Gaussian, drawn from --seed; "
          "cca: one projection per modality from the whitened cross-covariance of the pairs"),
         ("--rotation", str, "itq", "itq: iterative quantisation from the identity; none: no rotation (pca: PCAH, random: LSH)"),
         ("--itq-iters", int, 50, "ITQ iterations"),
         ("--cca-reg", float, 0.1, "ridge of the cca whitening, relative to the mean eigenvalue of a modality's covariance"),
         ("--fit-num", int, 0, "training items the fit reads, in loader order; 0: all of them")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
