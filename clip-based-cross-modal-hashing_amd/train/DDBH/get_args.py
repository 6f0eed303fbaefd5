"""DDBH flags (reference train/DDBH/get_args.py:7-15: the base flags and the save directory)."""
from argsbase import method_args


def get_args(main_args):
    return method_args(main_args, [])
