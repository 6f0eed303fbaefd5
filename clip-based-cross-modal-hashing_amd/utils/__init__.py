from .utils import *  # noqa: F401,F403
from .logger import get_logger, get_summary_writer  # noqa: F401
from .itq import fit_hash_heads  # noqa: F401
from .dch import fit_supervised_heads  # noqa: F401
