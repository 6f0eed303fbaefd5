"""DNPH flags (reference train/DNPH_TOMM/get_args.py): the base flags, and this build's choice of where the noise assignment runs."""
from argsbase import method_args

FLAGS = [("--noise-assign", str, "gpu", "Hungarian noise assignment of each step: gpu = exact solver on the device, no host round trip; "
          "host = numpy / scipy like upstream (this build)")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
