"""Cost of an intervention batch on the MI355X path.

Host logic only.  In the reference, ``Cost`` is an emukit ``Acquisition`` whose ``evaluate(x)`` adds up one
cost function per intervened variable, each applied to that variable's whole batch column
(/root/reference/src/utils_functions/cost_functions.py:5-17); with the graph classes' cost functions
(/root/reference/src/graphs/GraphInterface.py:46-50: fixed part plus, for "variable" costs, the sum of
|x| over everything passed in) this yields ONE scalar per batch, and emukit's quotient divides every
Expected-Improvement value of the batch by it.  The HIP sweep takes exactly that scalar
(``cbo_acq_sweep(..., cost, ...)``), so the quirk of summing |x| over the batch is kept.
"""
from __future__ import annotations

import numpy as np


class Cost:
    """Denominator of the acquisition ``EI / Cost`` for one exploration set."""

    has_gradients = True        # the reference reports gradients (all zero) so that L-BFGS may be used

    def __init__(self, costs_functions, evaluated_set):
        self.costs_functions = costs_functions      # mapping variable name -> callable(column) -> scalar
        self.evaluated_set = list(evaluated_set)    # variable names, in the column order of the candidates

    def per_variable(self, x):
        """The individual terms, one per intervened variable (column j of ``x`` belongs to variable j)."""
        x = np.asarray(x)
        return [self.costs_functions[name](x[:, j]) for j, name in enumerate(self.evaluated_set)]

    def evaluate(self, x):
        """Total cost of the batch ``x`` ((M, d)): a scalar (see the module docstring)."""
        return sum(self.per_variable(x), 0)

    def evaluate_with_gradients(self, x):
        """The reference returns zero gradients whatever the cost type (cost_functions.py:23-24)."""
        x = np.asarray(x)
        return self.evaluate(x), np.zeros(x.shape)


COST_MODES = ("batch", "pointwise")


def checked_cost_mode(cost_mode):
    """``cost_mode`` of the sweeps, the refinement, a path or an agent: ``"batch"`` (the reference's one scalar per batch,
    today's behaviour) or ``"pointwise"`` (every candidate over its own cost)."""
    if cost_mode not in COST_MODES:
        raise ValueError(f"cost_mode must be 'batch' or 'pointwise', not {cost_mode!r}")
    return cost_mode


class PointwiseCost(Cost):
    """The cost of every row of a batch by itself, ``c(x) = sum_k (fix_k + variable_k |x_k|)``: what the CBO
    papers divide the Expected Improvement by, where ``Cost`` hands the whole batch one scalar (the reference's quirk).  It
    needs a cost table that ``cost_structure`` recognises (``functools.partial(graphs.cost, fix, variable)`` per variable);
    anything else raises ``ValueError``.  ``acquisition / PointwiseCost(...)`` of the causal EI or its logarithm scores on
    the device through ``cbo_acq_sweep_pointcost``."""

    def __init__(self, costs_functions, evaluated_set):
        super().__init__(costs_functions, evaluated_set)
        from .causal_optimizer import cost_structure
        structure = cost_structure(self)
        if structure is None:
            raise ValueError("PointwiseCost needs a cost table of functools.partial(graphs.cost, fix, variable) entries, one "
                             "per variable of the evaluated set")
        self.fix, self.variable = structure
        if not float(self.fix.sum()) > 0.0:
            raise ValueError("PointwiseCost: the fixed costs must sum to a positive cost")

    def evaluate(self, x):
        """(M, 1): row i is ``one_row_cost(fix, variable, x[i])``, bit for bit."""
        from .causal_optimizer import one_row_cost
        x = np.asarray(x, dtype=np.float64)
        return np.array([[one_row_cost(self.fix, self.variable, row)] for row in x], dtype=np.float64).reshape(-1, 1)

    def evaluate_with_gradients(self, x):
        """The per-row costs and their own gradient, ``variable_k sign(x_k)`` (0 at 0)."""
        x = np.asarray(x, dtype=np.float64)
        return self.evaluate(x), self.variable[None, :].astype(np.float64) * np.sign(x)


def total_cost(intervention_variables, costs, x_new_dict):
    """Cost of performing one intervention, ``x_new_dict`` giving the value set for each intervened variable
    (used by ``CBO.compute_cost``, /root/reference/src/CBO.py:279-291)."""
    return float(sum(costs[name](x_new_dict[name]) for name in intervention_variables))
