"""Flags of the supervised training-free fit (no upstream counterpart).  The defaults are utils/dch.py's: choices made on a synthetic
fixture, not optima measured on a real dataset."""
from argsbase import method_args

FLAGS = [("--dch-iters", int, 10, "outer iterations: regressions, then rounds of coordinate descent over the bits"),
         ("--dch-rounds", int, 3, "Gauss-Seidel rounds over the bits per iteration"),
         ("--dch-lambda", float, 1.0, "ridge of the label regression W"),
         ("--dch-mu", float, 0.01, "weight of the two feature terms |B - X_m P_m|^2 against the label term"),
         ("--dch-reg", float, 0.1, "ridge of the feature regressions, relative to the mean eigenvalue of a modality's covariance"),
         ("--fit-num", int, 0, "training items the fit reads, in loader order; 0: all of them")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
