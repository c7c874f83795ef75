"""Test-only backend namespace for the `--use_8bit_optimizer` plumbing of main.py / unlearn.py without a GPU:
tests/oracle_backend.py with a FusedTrainer that records the keywords it is handed and stops the run there (`Reached`) -
what is under test is what the entry point asks of the trainer, not the training.  Never imported by the product."""
from oracle_backend import *  # noqa: F401,F403  (every name the entry points take from a backend)

CALLS = []


class Reached(Exception):
    """raised by FusedTrainer once its keywords are on record"""


class FusedTrainer:
    def __init__(self, model, scheduler, ema, **kw):
        CALLS.append(dict(kw, names=[n for n, _ in model.named_parameters()]))
        raise Reached()
