"""Greedy batch selection on the MI355X path: emukit's ``GreedyBatchPointCalculator`` (the Kriging believer).

emukit picks the acquisition's arg-max, adds it to the model as a fake observation whose ``y`` is the model's own
prediction there (``model.set_data`` -- one full refit per pick), picks again, ``batch_size`` times in all, and puts the
original data back.  Here the whole loop is ONE device call over the grid optimiser's resident grid
(``cbo_acq_sweep_batch``): the believed point is a candidate, so its column of ``L^-1 K*`` is already
resident, and its residual is zero, so only the candidates' variances change.  The model is never touched.
"""
from __future__ import annotations

import numpy as np

from .causal_acquisition_functions import AcquisitionQuotient, CandidateGrid, CausalExpectedImprovement
from .cost_functions import Cost


def check_batch_size(batch_size):
    if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive int, not {batch_size!r}")
    return int(batch_size)


class GreedyBatchPointCalculator:
    def __init__(self, model, acquisition, acquisition_optimizer, batch_size):
        """emukit's constructor.  ``acquisition``: a ``CausalExpectedImprovement`` -- or a ``CausalLogExpectedImprovement``,
        the same believer scored in log space (``cbo_acq_sweep_batch_logei``) -- bare or over a ``Cost``;
        ``acquisition_optimizer``: a ``CausalGradientAcquisitionOptimizer`` with ``anchors="grid"`` (no gradient stage is
        defined between picks).  Anything else raises ``ValueError``."""
        from .pointwise_acquisitions import CausalLogExpectedImprovement
        self.batch_size = check_batch_size(batch_size)
        numerator = acquisition.numerator if isinstance(acquisition, AcquisitionQuotient) else acquisition
        if not isinstance(numerator, (CausalExpectedImprovement, CausalLogExpectedImprovement)) or (
                isinstance(acquisition, AcquisitionQuotient) and not isinstance(acquisition.denominator, Cost)):
            raise ValueError("greedy batch selection is defined for the causal EI or its logarithm, bare or over a Cost, not for "
                             f"{type(acquisition).__name__}")
        if getattr(acquisition_optimizer, "anchors", "grid") != "grid":
            raise ValueError("greedy batch selection picks from the optimiser's grid: anchors must be 'grid'")
        self.model = model
        self.acquisition = acquisition
        self.acquisition_optimizer = acquisition_optimizer

    def compute_next_points(self, loop_state=None, context=None, update_incumbent=False):
        """(batch_size, d): the batch, row t being pick t.  ``loop_state`` and ``context`` are accepted as emukit passes
        them and not used."""
        opt = self.acquisition_optimizer
        model = self.acquisition.model
        if opt._grid is None or opt._grid_model is not model:
            if opt._grid is not None:
                opt._grid.close()
            opt._grid, opt._grid_model = CandidateGrid(opt.candidates(), model), model
        grid = opt._grid
        res = self.acquisition.sweep_batch(grid, self.batch_size, update_incumbent=update_incumbent)
        self.last_result = res
        return grid.points[res["best_idx"] - grid.index_offset].copy()
