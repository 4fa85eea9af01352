"""Mirror of the reference package ``src.utils_functions`` for the names on the hot path
(/root/reference/src/utils_functions/__init__.py star-imports the same modules)."""
from .causal_acquisition_functions import (AcquisitionQuotient, CausalExpectedImprovement, CandidateGrid,  # noqa: F401
                                           PointCostQuotient)
from .causal_optimizer import CausalGradientAcquisitionOptimizer  # noqa: F401
from .constrained import (AcquisitionProduct, ConstrainedLogExpectedImprovement,  # noqa: F401
                          ProbabilityOfFeasibility)
from .cost_functions import Cost, PointwiseCost, total_cost  # noqa: F401
from .greedy_batch import GreedyBatchPointCalculator  # noqa: F401
from .integrated_hyper import IntegratedHyperParameterAcquisition, hmc_sample  # noqa: F401
from .integrated_variance import IntegratedVarianceReduction  # noqa: F401
from .max_value_entropy import MaxValueEntropySearch  # noqa: F401
from .pointwise_acquisitions import (CausalLogExpectedImprovement, CausalMeanPluginExpectedImprovement,  # noqa: F401
                                     CausalNegativeLowerConfidenceBound, CausalProbabilityOfImprovement,
                                     LogAcquisitionQuotient, ModelVariance)
from .utils import (compute_coverage, find_current_global, find_next_y_point, find_next_y_points,  # noqa: F401
                    fit_gaussian_process, fit_gaussian_processes, update_hull)
from .graph_functions import (AdditiveSEM, Term, compute_interventions, get_parameter_space, intervene_dict,  # noqa: F401
                              sample_from_model)
