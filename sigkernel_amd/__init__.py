"""sigkernel_amd -- MI355X-native signature-PDE-kernel engine.

Drop-in for the ``SigKernel.compute_kernel / compute_Gram / compute_mmd`` path of
crispitagorico/sigkernel: Python host code on PyTorch-ROCm calling hand-written HIP kernels
(gfx950) through the C ABI in ``include/sigkernel_amd.h``.
"""
from ._routes import routes
from .static_kernels import (CEXP, Linear_ID_Kernel, LinearKernel, RBF_CEXP_Kernel, RBF_ID_Kernel, RBF_SQR_Kernel, RBFKernel,
                             cos_exp_kernel)
from .sigkernel import SigKernel, SigKernelStream, _SigKernel, _SigKernelGram, k_kgrad, pad_paths
from .stats import SigCHSIC, c_alpha, hypothesis_test
from .transforms import AddTime, LeadLag, add_time, lead_lag, transform
from .truncated import (truncated_sig_kernel, truncated_sig_kernel_paired, truncated_sig_kernel_levels, truncated_from_levels,
                        truncated_robust_scales, TruncatedSigKernel)

__all__ = ["SigKernel", "SigKernelStream", "LinearKernel", "RBFKernel", "_SigKernel", "_SigKernelGram", "hypothesis_test", "SigCHSIC",
           "c_alpha", "transform", "add_time", "lead_lag", "AddTime", "LeadLag", "k_kgrad", "routes", "Linear_ID_Kernel", "RBF_ID_Kernel",
           "RBF_CEXP_Kernel", "RBF_SQR_Kernel", "CEXP", "cos_exp_kernel", "truncated_sig_kernel", "truncated_sig_kernel_paired", "truncated_sig_kernel_levels",
           "truncated_from_levels", "truncated_robust_scales", "TruncatedSigKernel", "pad_paths"]
__version__ = "0.1.0"
