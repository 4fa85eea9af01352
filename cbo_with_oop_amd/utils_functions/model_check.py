"""Checking a posterior before trusting it: leave-one-out cross-validation of many models in one device call.

In causal BO every exploration set can be modelled with the do-calculus prior (``create_causal_gp``) or without it
(``create_non_causal_gp``).  The prior mean comes from observational data and can be wrong, and at 10-50 points the
marginal likelihood says little.  The LOO pseudo-likelihood (Rasmussen & Williams 5.4.2) of both models, from the
factor each already implies, says which of the two predicts the points it has not seen better."""
import ctypes

import numpy as np

from .. import _lib


def loo_scores(models):
    """The LOO pseudo-likelihood (``loo_score()``) of every model, ONE ``cbo_gp_loo_batch`` call: every fp64 model of at
    most 128 observations is answered inside one launch, fitted or not, and left as it was; larger models are fitted
    first and answered one by one.  A model whose Ky is not positive definite even with the jitchol ladder's jitter
    raises LinAlgError, as the model alone does."""
    models = list(models)
    if not models:
        return []
    lib = _lib.load()
    for m in models:
        if not m.small:
            m.ensure_fitted()
    k = len(models)
    handles = (ctypes.c_void_p * k)(*[m._handle for m in models])
    sums = np.zeros(k)
    status = np.zeros(k, dtype=np.int32)
    _lib.check(lib.cbo_gp_loo_batch(k, handles, _lib.dptr(sums), None, status.ctypes.data_as(_lib.c_int_p)))
    for rc in status:
        _lib.check(int(rc))
    return [float(v) for v in sums]


def prefer_causal_prior(causal_models, plain_models):
    """Per exploration set: does the model with the do-calculus prior have the higher LOO pseudo-likelihood than the one
    without?  One device call for all 2 S models."""
    causal_models, plain_models = list(causal_models), list(plain_models)
    if len(causal_models) != len(plain_models):
        raise ValueError("one causal and one plain model per exploration set")
    scores = loo_scores(causal_models + plain_models)
    s = len(causal_models)
    return [scores[i] > scores[s + i] for i in range(s)]
