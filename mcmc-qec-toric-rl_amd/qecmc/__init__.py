"""qecmc -- MI355X-native MCMC equivalence-class sampler (host-side mirror of the
reference's Toric_code / Chain / Ladder / PTEQ API over the libqecmc C-ABI)."""
from ._lib import QecmcError, device_count, lib, dev_flags, use_library
from ._lib import TORIC, XZZX, ROTATED, PLANAR, SCANS
from .toric_model import Toric_code
from .xzzx_model import xzzx_code
from .rotated_surface_model import RotSurCode
from .planar_model import Planar_code
from .mcmc import Chain, Ladder, Chain_xyz
from .mcmc_biased import Chain_biased, Ladder_biased
from .decoders import PTEQ, PTDC, STDC, STRC, PTRC, STDC_general_noise, STDC_general_noise_shortest, STDC_Nall_n_alpha, single_temp, pteq_batch, ptdc_batch, ptdc_distribution, percent_from_counts
from .mcmc_alpha import Chain_alpha, Ladder_alpha
from .decoders_biasednoise import PTEQ_biased, PTEQ_alpha, PTEQ_alpha_with_shortest, pteq_shortest_batch, shortest_distribution
from .syndrome_lift import chains_from_syndromes
from .syndrome_corrections import corrections
from .exact import (coset_enumerator, class_weights, depolarizing_weight, biased_weight, alpha_weight, exact_class_probabilities,
                    exact_rung_observables, class_sweep, class_sweep_cut, sweep_cut_info, class_sweep_tiled, sweep_tiled_info, depolarizing_w4, biased_w4, alpha_w4,
                    class_sweep_site, resolve_site_method, exact_site_probabilities, depolarizing_site_w4, biased_site_w4, erasure_site_w4,
                    class_minplus, min_weight_classes, shortest_class_law, shortest_chains, min_weight_corrections,
                    class_minplus_site, shortest_chains_site, min_weight_classes_site, min_weight_corrections_site, erasure_site_costs, llr_site_costs,
                    sample_chains, sample_chains_site, sample_posterior, posterior_error_counts,
                    class_marginals, class_marginals_site, posterior_marginals, exact_error_counts,
                    class_minplus_tiled, class_minplus_tiled_site, shortest_chains_tiled, shortest_chains_tiled_site,
                    sample_chains_tiled, sample_chains_tiled_site, sample_tiled_info)

__all__ = ["QecmcError", "device_count", "lib", "TORIC", "XZZX", "ROTATED", "PLANAR", "Toric_code", "xzzx_code", "RotSurCode", "Planar_code",
           "Chain", "Ladder", "Chain_xyz", "Chain_biased", "Ladder_biased", "Chain_alpha", "Ladder_alpha", "PTEQ", "PTDC", "STDC", "STRC", "PTRC", "STDC_general_noise", "STDC_general_noise_shortest", "STDC_Nall_n_alpha", "single_temp", "PTEQ_biased", "PTEQ_alpha", "PTEQ_alpha_with_shortest", "pteq_shortest_batch", "shortest_distribution", "ptdc_batch", "ptdc_distribution", "pteq_batch", "percent_from_counts", "chains_from_syndromes", "corrections",
           "coset_enumerator", "class_weights", "depolarizing_weight", "biased_weight", "alpha_weight", "exact_class_probabilities", "exact_rung_observables",
           "class_sweep", "class_sweep_cut", "sweep_cut_info", "class_sweep_tiled", "sweep_tiled_info", "depolarizing_w4", "biased_w4", "alpha_w4",
           "class_sweep_site", "resolve_site_method", "exact_site_probabilities", "depolarizing_site_w4", "biased_site_w4", "erasure_site_w4",
           "class_minplus", "min_weight_classes", "shortest_class_law", "shortest_chains", "min_weight_corrections",
           "class_minplus_site", "shortest_chains_site", "min_weight_classes_site", "min_weight_corrections_site", "erasure_site_costs", "llr_site_costs",
           "sample_chains", "sample_chains_site", "sample_posterior", "posterior_error_counts",
           "class_marginals", "class_marginals_site", "posterior_marginals", "exact_error_counts",
           "class_minplus_tiled", "class_minplus_tiled_site", "shortest_chains_tiled", "shortest_chains_tiled_site",
           "sample_chains_tiled", "sample_chains_tiled_site", "sample_tiled_info"]
