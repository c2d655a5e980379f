"""Host-side helpers of the training loops and the device-resident evaluation side-car."""
from .batches import batches, rows_on_device
from .energy_utils import class_free_energies, rbm_free_energy
from . import probe_utils
from . import conditional_steps
from . import imdbn_logging
from . import bimodal_logging
from . import cross_eval
from . import likelihood
from . import retrieval

__all__ = ["batches", "rows_on_device", "rbm_free_energy", "class_free_energies", "probe_utils", "conditional_steps", "imdbn_logging", "bimodal_logging",
           "cross_eval", "likelihood", "retrieval"]
