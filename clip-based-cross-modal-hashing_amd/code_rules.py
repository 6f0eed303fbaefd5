"""What turns a method model's output into its hash code in {-1, 0, +1}: stated once, for the trainers' evaluation loops
(train/base.py::get_code*, reference train/base.py:130-223) and for the query front end (query.py)."""
import torch

import cmh_native as N


def sign_code(out) -> torch.Tensor:
    """sign() of the tanh head's output (DSPH, DNpH, DMsH_LN, DHaPH, DDBH, ITQ, DCH, DJSRH, MSCH, CPFH, DWSH; reference train/base.py:130-148)."""
    return N.sign_codes(out)


def pair_argmax_code(out) -> torch.Tensor:
    """argmax over each pair of probabilities; index 0 -> -1, 1 -> +1 (DCHMT; reference train/base.py:150-158).  `out`: the head's
    list of [B, 2] pairs, or their concatenation [B, 2K]."""
    p = torch.cat(out, dim=-1) if isinstance(out, (list, tuple)) else out
    return N.pair_argmax_codes(p)


def first_sign_code(out) -> torch.Tensor:
    """sign() of the first output; the second is the class logits (DNPH; reference train/base.py:206-223)."""
    return N.sign_codes(out[0])


CODE_RULES = {"DSPH": sign_code, "DNpH": sign_code, "DMsH_LN": sign_code, "DHaPH": sign_code, "DDBH": sign_code, "ITQ": sign_code,
              "DCH": sign_code, "DJSRH": sign_code, "MSCH": sign_code, "CPFH": sign_code, "DWSH": sign_code,
              "DCHMT": pair_argmax_code, "DNPH": first_sign_code}


def soft_output(out) -> torch.Tensor:
    """The tanh head's output itself: sign_code writes its sign."""
    return out.float()


def pair_margin(out) -> torch.Tensor:
    """p[..., 1] - p[..., 0] of each probability pair: positive exactly where pair_argmax_code picks index 1 (+1), negative where
    it picks index 0 (-1); 0 on a tie, which the argmax gives to index 0."""
    p = torch.cat(out, dim=-1) if isinstance(out, (list, tuple)) else out
    p = p.float().reshape(p.shape[0], -1, 2)
    return p[..., 1] - p[..., 0]


def first_soft_output(out) -> torch.Tensor:
    """The first output itself; the second is the class logits (DNPH)."""
    return out[0].float()


# The real-valued output behind each rule of CODE_RULES, for soft queries (utils/retrieval.py::soft_topk): wherever it is
# non-zero, its sign is the code the method's rule writes.
SOFT_RULES = {"DSPH": soft_output, "DNpH": soft_output, "DMsH_LN": soft_output, "DHaPH": soft_output, "DDBH": soft_output,
              "ITQ": soft_output, "DCH": soft_output, "DJSRH": soft_output, "MSCH": soft_output, "CPFH": soft_output, "DWSH": soft_output,
              "DCHMT": pair_margin, "DNPH": first_soft_output}


def code_rule(method):
    """The rule TrainBase._codes_for_eval applies for `method` (sign_code for every method without a rule of its own)."""
    return CODE_RULES.get(method, sign_code)


def soft_rule(method):
    """The soft output that goes with code_rule(method)."""
    return SOFT_RULES.get(method, soft_output)
