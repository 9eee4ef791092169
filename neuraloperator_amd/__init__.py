"""neuraloperator_amd -- MI355X-native SpectralConv engine (drop-in ``conv_module`` for FNO/TFNO).

Only the hot path of neuralop.layers.spectral_convolution lives here:
hand-written HIP kernels behind a C-ABI (include/sc_engine.h, neuraloperator_amd/csrc) and
the Python module that mirrors the reference's plug-in interface.
"""
from .spectral_conv import BaseSpectralConv, SpectralConv  # noqa: F401
from .factorized import CPWeight, DenseWeight, SpectralWeight, TTWeight, TuckerWeight  # noqa: F401
from .optim import AdamW  # noqa: F401
from .galore import TensorGaLoreProjector  # noqa: F401
from .spherical import SHT, SphericalConv  # noqa: F401
from .harmonics import InverseRealSHT, RealSHT, install_torch_harmonics  # noqa: F401
from .differentiation import (FiniteDiff, FourierDiff, NonUniformFD, get_non_uniform_fd_weights,  # noqa: F401
                              non_uniform_fd)
from .losses import H1Loss, LpLoss  # noqa: F401
from .gno import GNOBlock, IntegralTransform, NeighborSearch, segment_csr  # noqa: F401
from .differential_conv import FiniteDifferenceConvolution  # noqa: F401
from .discrete_continuous_convolution import (DiscreteContinuousConv2d, DiscreteContinuousConvTranspose2d,  # noqa: F401
                                              EquidistantDiscreteContinuousConv2d,
                                              EquidistantDiscreteContinuousConvTranspose2d)
from .local_no_block import LocalNOBlocks  # noqa: F401
from .attention import AttentionKernelIntegral, RotaryEmbedding2D  # noqa: F401
from .spectral_projection import HelmholtzProjection, spectral_projection_divergence_free  # noqa: F401
from .graph import GraphedStep, capture_step  # noqa: F401

__version__ = "0.1.0"
