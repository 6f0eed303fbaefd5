"""Supervised training-free codes from a stock CLIP checkpoint (no upstream counterpart): discrete cross-modal hashing (DCH, Xu et
al., TIP 2017) on the towers' own features.  train() makes one pass over the train loader without gradients, keeps the features and
the labels of the fit set on the GPU, fits the two heads (utils/dch.py, csrc/dch.hip), writes them into the model, saves model-0.pth
and runs the usual validation.  The checkpoint has DSPH's keys: it loads as `--method DCH`, as `--method ITQ` and as `--method DSPH`."""
import time

from model.DCH import MDCH
from train.fit_base import FitTrainer
from utils.dch import fit_from_moments, supervised_moments
from utils.itq import load_heads
from .get_args import get_args


class DCHTrainer(FitTrainer):
    name, model_class = "DCH", MDCH

    def __init__(self, args, rank=0):
        super().__init__(get_args(args), rank)

    @staticmethod
    def check_args(args):
        if args.dch_iters < 0 or args.dch_rounds < 1:
            raise ValueError(f"DCH: --dch-iters {args.dch_iters} / --dch-rounds {args.dch_rounds}: need iters >= 0 and rounds >= 1")
        if not (args.dch_lambda > 0.0 and args.dch_mu >= 0.0 and args.dch_reg > 0.0):
            raise ValueError(f"DCH: --dch-lambda {args.dch_lambda} / --dch-mu {args.dch_mu} / --dch-reg {args.dch_reg}: "
                             f"need lambda > 0, mu >= 0 and reg > 0")

    def fit(self):
        began = time.time()
        self.change_state(mode="valid")
        Fi, Ft, Y, moments = self.collect_features(keep_labels=True)
        a = self.args
        fit = fit_from_moments(Fi, Ft, Y, supervised_moments(moments), a.output_dim, a.dch_iters, a.dch_rounds, a.dch_lambda, a.dch_mu,
                               a.dch_reg)
        load_heads(self.model, fit)
        self.total_time += time.time() - began
        obj = [float(v) for v in fit["objective"].cpu()]                 # the fit's reads: after the last launch
        flips, margins, info = fit["flips"].cpu().tolist(), fit["min_margin"].cpu().tolist(), fit["solve_info"].cpu().tolist()
        self.logger.info(f">>>>>> fit: DCH on {Fi.shape[0]} pairs, D = {Fi.shape[1]}, C = {Y.shape[1]}, bits = {a.output_dim}, "
                         f"lambda = {a.dch_lambda:g}, mu = {a.dch_mu:g}, reg = {a.dch_reg:g} / D, scale = {float(fit['scale']):.6g}, "
                         f"time: {self.total_time}")
        self.logger.info(f">>>>>> Jacobi sweeps (S_ii, S_tt, C): {fit['eigh_sweeps']}, converged: {fit['eigh_converged_each']}")
        for it, v in enumerate(obj):
            tail = f", flips per round {flips[it]}, min margin {margins[it]:.3e}" if it < len(flips) else " (the codes returned)"
            self.logger.info(f">>>>>> objective[{it}]: {v!r}{tail}")
        if any(info):
            self.logger.warning(f">>>>>> label regression: a pivot that was not positive (solve_info {info}); W was zeroed there")
        self.last_fit = fit
        return fit
