"""Training-free codes from a stock CLIP checkpoint (no upstream counterpart): LSH, PCAH and ITQ (Gong & Lazebnik, CVPR 2011) on
the towers' own features, and with --projection cca the paper's cross-modal variant (one projection per modality from the whitened
cross-covariance of the pairs).  train() makes one pass over the train loader without gradients, keeps the features on the GPU, fits the
two heads (utils/itq.py, csrc/itq.hip), writes them into the model, saves model-0.pth and runs the usual validation.  Labels are
read by the evaluation alone.  The checkpoint has DSPH's keys: it loads as `--method ITQ` and as `--method DSPH`."""
import time

from model.ITQ import MITQ
from train.fit_base import FitTrainer
from utils.itq import PROJECTIONS, ROTATIONS, fit_from_moments, load_heads
from .get_args import get_args


class ITQTrainer(FitTrainer):
    name, model_class = "ITQ", MITQ

    def __init__(self, args, rank=0):
        super().__init__(get_args(args), rank)

    @staticmethod
    def check_args(args):
        if args.projection not in PROJECTIONS or args.rotation not in ROTATIONS:
            raise ValueError(f"ITQ: --projection {args.projection} / --rotation {args.rotation}: one of {PROJECTIONS} and one of {ROTATIONS}")
        if args.projection == "cca" and not args.cca_reg > 0.0:
            raise ValueError(f"ITQ: --cca-reg {args.cca_reg}: the ridge must be positive")

    def fit(self):
        began = time.time()
        self.change_state(mode="valid")
        cca = self.args.projection == "cca"
        Fi, Ft, _, moments = self.collect_features(cross=cca)
        fit = fit_from_moments(Fi, Ft, moments.finish_cca() if cca else moments.finish(), self.args.output_dim, self.args.projection,
                               self.args.rotation, self.args.itq_iters, seed=self.args.seed, reg=self.args.cca_reg)
        load_heads(self.model, fit)
        self.total_time += time.time() - began
        obj = [float(v) for v in fit["objective"].cpu()]
        self.logger.info(f">>>>>> fit: {self.args.projection}+{self.args.rotation} on {Fi.shape[0]} pairs, D = {Fi.shape[1]}, "
                         f"bits = {self.args.output_dim}, scale = {float(fit['scale']):.6g}, time: {self.total_time}")
        if "evals" in fit:
            ev = fit["evals"].cpu()
            kept = float(ev[:self.args.output_dim].sum() / ev.sum())
            self.logger.info(f">>>>>> eigenvalue share kept: {kept:.6f} (Jacobi sweeps: {fit['eigh_sweeps']}, converged: {fit['eigh_converged']})")
        if cca:
            kept = fit["correlations"][:self.args.output_dim].cpu()
            self.logger.info(f">>>>>> canonical correlations kept: first {float(kept[0]):.6f}, last {float(kept[-1]):.6f}, mean {float(kept.mean()):.6f} "
                             f"(ridge {fit['reg']:g} / D; Jacobi sweeps: {fit['eigh_sweeps']}, converged: {fit['eigh_converged_each']})")
        for it, v in enumerate(obj):
            self.logger.info(f">>>>>> objective[{it}]: {v!r}")
        self.last_fit = fit
        return fit
