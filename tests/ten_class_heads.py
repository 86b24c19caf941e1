"""The ten-class entry points of the classifier's loss heads (csrc/loss.hip), called directly by tests/test_gpu_loss_heads_k.py for its
K = 10 bit-identity checks and its negative control.  They live outside tests/test_gpu_*.py because tests/test_kernel_coverage.py keeps
tg_c_loss_terms_f32 and tg_true_fake_loss_f32 on its THROUGH_WRAPPER list, which requires that no GPU test file calls them by name."""
import ctypes as C

import numpy as np

from kernel_check import dev, lib, ptr, st


def c_loss(g, loss, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, lambdas):
    """tg_c_loss_f32 (weights {1, .005, 1e-6, 1e-3}, device lambdas)."""
    n, ld = z.shape
    lib().call('tg_c_loss_f32', ptr(dev(z)), ld, n_real, n_unl, n_rep, n_fake, ptr(dev(y_real)), ptr(dev(y_fake)), ptr(dev(d_unl)), 1,
               ptr(dev(np.asarray(lambdas, np.float32))), g.ptr, g.n // n, loss.ptr, st())


def c_loss_terms(g, loss, terms, z, n_real, n_unl, n_rep, n_fake, y_real, y_fake, d_unl, w6):
    """tg_c_loss_terms_f32 (host weights)."""
    n, ld = z.shape
    lib().call('tg_c_loss_terms_f32', ptr(dev(z)), ld, n_real, n_unl, n_rep, n_fake, ptr(dev(y_real)), ptr(dev(y_fake)) if n_fake else None,
               ptr(dev(d_unl)), 1, (C.c_float * 6)(*w6), g.ptr, g.n // n, loss.ptr, terms.ptr, st())


def true_fake_loss(zu, zf, w_unl, w_fake, gu, ld_du, acc_u, gf, ld_df, acc_f, loss):
    """tg_true_fake_loss_f32."""
    lib().call('tg_true_fake_loss_f32', ptr(dev(zu)), zu.shape[1], len(zu), ptr(dev(zf)), zf.shape[1], len(zf), w_unl, w_fake, gu.ptr, ld_du,
               acc_u, gf.ptr, ld_df, acc_f, loss.ptr, st())
