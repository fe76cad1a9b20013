"""emdenoise: MI355X-native (gfx950) implementation of the CNN micrograph-denoising hot path of
Jeffrey-Ede/AI-CV-Automation-Elect-Micr, behind the reference's own Python call surface.

Python here is host logic only (shapes, buffers, streams); all arithmetic runs in hand-written
HIP kernels reached through the C ABI of libemdenoise.so (include/emdenoise.h).
"""
from . import _lib  # noqa: F401
from .kernel_denoiser import KernelParams, Micrograph_Autoencoder, kernel_denoise  # noqa: F401
from . import affine, autoencoder, autoencoder_trainer, denoiser, diversity, dose, exitwave, filters, focus, gan, graphed, harvest, input_pipeline, k_trainer, kernel_denoiser, metrics, ops, psiart, resample, spectral, streams, tf_checkpoint, tiling, train_ops, trainer, xception  # noqa: F401
from .denoiser import Denoiser, DenoiserEngine, architecture, synthetic_weights  # noqa: F401
from .trainer import DenoiserTrainer, get_model_fn  # noqa: F401
from .k_trainer import KernelDenoiserTrainer, PAIR_PRESET, distill, k_record_parser, make_pairs, s_record_parser  # noqa: F401
from .autoencoder_trainer import AutoencoderTrainer  # noqa: F401
from .metrics import ms_ssim, psnr, ssim, ssim_loss, tf_ms_ssim, tf_ssim  # noqa: F401
from .filters import baseline_table  # noqa: F401

__all__ = ["KernelParams", "Micrograph_Autoencoder", "kernel_denoise", "KernelDenoiserTrainer", "AutoencoderTrainer", "make_pairs", "distill",
           "PAIR_PRESET", "ssim", "ms_ssim", "psnr", "ssim_loss", "tf_ssim", "tf_ms_ssim", "filters", "baseline_table", "harvest", "exitwave", "affine", "psiart", "resample", "focus", "dose", "diversity", "spectral"]
