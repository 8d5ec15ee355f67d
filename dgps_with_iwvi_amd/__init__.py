"""MI355X-native importance-weighted ELBO hot path of hughsalimbeni/DGPs_with_IWVI.

Module names mirror the reference package (``layers``, ``models``, ``temp_workaround``); the
GPflow-1.x pieces the reference takes from gpflow live in ``kernels``, ``features``,
``mean_functions``, ``likelihoods`` and ``settings``.  All arithmetic is in
``csrc/libiwvi_hip.so`` (hand-written gfx950 HIP behind the C-ABI of include/iwvi_hip.h).
"""
import os as _os

# Kernel arguments in device memory (ROCm runtime switch, read when HIP initialises): the layer launch carries ~5 KB of arguments and
# reads them through the scalar cache first thing; from host-visible memory that first read is a PCIe round trip (measured: bench.py,
# `no_dev_kernarg`).  Set here so that what a user of the package runs is what bench.py times -- it takes effect when this import
# comes before the process's first HIP call (safest: before `import torch`); an explicit HIP_FORCE_DEV_KERNARG in the environment wins.
# It is a process-wide runtime switch (torch's and RCCL's kernels in this process see it too, child processes inherit it): set
# IWVI_NO_ENV_DEFAULTS=1 to keep the package from touching the environment at all.
if not _os.environ.get("IWVI_NO_ENV_DEFAULTS"):
    if "HIP_FORCE_DEV_KERNARG" not in _os.environ:
        _os.environ["HIP_FORCE_DEV_KERNARG"] = "1"
        import sys as _sys
        _t = _sys.modules.get("torch")
        if _t is not None and _t.cuda.is_initialized():          # too late for this process: say so instead of silently doing nothing
            import warnings as _w
            _w.warn("dgps_with_iwvi_amd was imported after HIP initialised: HIP_FORCE_DEV_KERNARG=1 (device-resident kernel arguments, "
                    "~1 us per layer launch) is not in effect; import the package before the first GPU call or export the variable")

from . import settings  # noqa: F401
from . import features, kernels, likelihoods, mean_functions  # noqa: F401
from . import layers, models, temp_workaround  # noqa: F401
from .layers import Encoder, GPLayer, LatentVariableLayer, RegularizerType  # noqa: F401
from .models import Bound, DGP_IWVI, DGP_VI  # noqa: F401
from .temp_workaround import (SharedMixedMok, gauss_kl,  # noqa: F401
                              independent_multisample_sample_conditional,
                              multisample_sample_conditional)

__all__ = ["settings", "features", "kernels", "likelihoods", "mean_functions", "layers", "models",
           "temp_workaround", "Encoder", "GPLayer", "LatentVariableLayer", "RegularizerType",
           "Bound", "DGP_IWVI", "DGP_VI", "SharedMixedMok", "gauss_kl",
           "independent_multisample_sample_conditional", "multisample_sample_conditional"]
