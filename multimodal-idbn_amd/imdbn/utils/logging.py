"""Alias of ``imdbn.utils.imdbn_logging`` (the reference ships the same module under both names): the same function objects."""
from .imdbn_logging import *  # noqa: F401,F403
from .imdbn_logging import __all__  # noqa: F401
