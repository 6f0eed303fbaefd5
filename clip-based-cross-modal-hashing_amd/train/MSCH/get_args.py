"""MSCH flags.  Margin and scale are the reference's (train/DPSIH/get_args.py: margin 0.25; train/DPSIH/Loss.py:62: the factor 100);
`all` is the only rule the reference's trainer ever reaches (train/MSCH/loss.py); the symmetric pair is this build's addition."""
from argsbase import method_args, str2bool

MININGS = ("all", "semi-hard")
FLAGS = [("--msc-margin", float, 0.25, "margin m of the triplet loss: a triplet is active when s_an - s_ap <= m"),
         ("--msc-scale", float, 100.0, "factor on the sum of the pairs' losses"),
         ("--msc-mining", str, "all", "all: every triplet within the margin; semi-hard: only those with 0 < s_an - s_ap"),
         ("--msc-symmetric", str2bool, False, "also add the text -> image loss as a fourth pair (not upstream's; nothing is divided)")]


def get_args(main_args):
    return method_args(main_args, FLAGS)
