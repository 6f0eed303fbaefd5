"""Model of the supervised training-free method (DCH; no upstream counterpart): MITQ under the method's own name - Baseclip with
LinearHash heads and DSPH's keys, so its checkpoints also load as DSPH and as ITQ.  The heads are written by the fit (utils/dch.py),
never trained."""
from model.ITQ import MITQ


class MDCH(MITQ):
    pass
