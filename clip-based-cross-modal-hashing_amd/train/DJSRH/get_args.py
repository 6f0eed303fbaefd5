"""DJSRH flags (no upstream counterpart).  The five scalars' defaults are the paper's MIRFlickr settings as far as they are recalled:
choices, not measured optima."""
from argsbase import method_args

INIT_HEADS = ("random", "itq", "cca")
FLAGS = [("--djsrh-beta", float, 0.9, "weight of the image features' cosine in the target; 1 - beta is the captions'"),
         ("--djsrh-eta", float, 0.4, "share of the second-order term St St^T / B in the target"),
         ("--djsrh-mu", float, 1.5, "scale of the target"),
         ("--djsrh-lambda1", float, 0.1, "weight of the image-image term"),
         ("--djsrh-lambda2", float, 0.1, "weight of the text-text term"),
         ("--init-heads", str, "random", "random: the heads as drawn; itq / cca: fitted on the cached stock features before the first "
          "step (utils/itq.py: pca + itq, or one projection per modality from the pairs' cross-covariance + itq)")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
