"""lam_slide_amd: MI355X (gfx950) implementation of LaM-SLidE's second-stage latent SiT sampling path.

Public surface (mirrors the reference's for this path only):
  LatentSIV3                       <- src.models.components.latent.latent_si_v31.LatentSIV3
  CreateTransport, Transport, Sampler, ModelType, PathType
                                   <- src.modules.transport (samplers, and Transport.training_losses without gradients)
  SecondStageSampler, setup_conditioning, sample_sharded
                                   <- SecondStageCondLightningBase.{sample, setup_conditioning} + batch sharding
  Stage1Decoder                    <- first_stage.decode = Decoder(post_quant(latents), entities) (frozen, after the sampler)
  Stage1Encoder                    <- quant(Encoder(prepare_inputs(batch), entities, mask)) (frozen, before the sampler)
  best_of_k_errors, min_ade_fde    <- the K-sample test loops + _compute_errors (second_stage/pedestrian.py:178-212)
  RolloutSampler, sample_rollout   <- SIAtom14SamplingWrapper.{create_batch, sample_rollout} (modules/sampling.py:16-63)
  Loss, geom_losses, geom_loss_sums
                                   <- second_stage/{md17,nba,pedestrian}.Loss with calc_additional_losses: MaskedMSELoss, MaskedNormLoss
                                      and InterDistanceLoss of the decoded positions on the device (losses.py)
  PeptideLoss, peptide_losses, peptide_loss_sums
                                   <- second_stage/peptide.Loss with calc_additional_losses: those three of the atom14 positions plus
                                      the frame-local position loss and the torsion loss on the device (peptide_loss.py)
  displacement_errors, displacement_rows, DisplacementMeter
                                   <- the ADE / FDE lines of validation_step, the best-of-K tail of test_step and the epoch means of
                                      second_stage/{md17,nba,pedestrian}.py on the device (metrics.py)
  TorsionStats, dihedral_angles, angle_histograms, js_distance, lagged_products, decorrelation
                                   <- the torsion statistics of eval_peptide.analyze_trajectory (histograms of every torsion and of
                                      chosen pairs, Jensen-Shannon distances to the MD reference, decorrelation curves) of the sampled
                                      atom14 positions on the device (torsion_stats.py)
  TicaModel, tica_jsd, lagged_moments, tica_covariances, assign_centers, transition_counts, metastable_jsd, ...
                                   <- the TICA and Markov-state half of analyze_trajectory (eval_peptide.py:189-288): the lagged second
                                      moments and the projection of a TICA model, TICA-0 / TICA-0,1 on the joint range, nearest-centre
                                      labels, state occupancies and transition counts on the device (tica.py)
  kmeans_fit, nearest_rows, KMeansResult, fit_microstates
                                   <- k-means fitting on the device (kmeans.py): ``analysis.get_kmeans`` of the peptide evaluation and the
                                      ``post_process`` branch of the NBA / pedestrian test_step (``displacement_errors(post_process=True)``)
  estimate_markov_model, MarkovModel, active_set, pcca_assignments, markov_state_block
                                   <- the Markov state models of analyze_trajectory (eval_peptide.py:245-288, modules/analysis.py:47-56): the
                                      largest connected set, the reversible maximum-likelihood estimate of the microstate, coarse and
                                      trajectory models on the device, PCCA+ assignments by the inner simplex algorithm on the host (msm.py)
  traj_analysis, StructureTables, pair_distances, ca_frame_stats, tica_features, density_js, joint_density_js, ...
                                   <- the structure statistics SIAtom14SampleCallback logs per validation epoch (utils/traj_utils.py
                                      traj_analysis: ramachandran_js, pwd_js, rg_js, tic_js, tic2d_js, val_ca, rmse_contact) of the sampled
                                      atom14 positions on the device (structure_stats.py)
  run_tica, koopman_weights, weighted_moments, WideTicaModel, KoopmanWeights
                                   <- ``tica_utils.run_tica``: the Koopman-reweighted TICA over ``tica_features`` (129 .. 2048 columns) on the
                                      device - ``traj_analysis(..., tica_lagtime=)`` gives tic_js / tic2d_js from positions alone
                                      (koopman_tica.py)
  Stage1Autoencoder, class_losses, class_loss_sums, ClassMeter, first_stage.{MD17Loss, PedestrianLoss, NBALoss, PeptideLoss}
                                   <- first-stage validation (first_stage/{md17,pedestrian,nba,peptide}.py model_step / validation_step):
                                      encode -> decode with every output head from one trunk (``Stage1Decoder.decode_heads``), the four
                                      first-stage ``Loss`` classes with their cross-entropy terms and the accuracy / precision / recall
                                      counts on the device (first_stage.py)
  superpose.superpose, center_coordinates, rmsd, rmsf, superpose_atom14, create_trajectory
                                   <- rigid superposition of the sampled positions on the device (superpose.py): the Kabsch fit mdtraj's
                                      ``traj.superpose`` runs before a trajectory is written (eval_peptide.py:347) or analysed
                                      (utils/traj_utils.py create_trajectory), its RMSD, and the per-atom RMSF.  ``superpose`` names the
                                      module here; the function is ``superpose.superpose``
  install()                        <- rebinds the reference's module-level ``Sampler`` (lightning_base.py:10); see dropin.py
The compute lives in liblamslide_hip.so (include/lsl_api.h); build it with ``__graft_entry__.build()``.
"""
from . import _lib, dropin
from .dropin import install, uninstall
from .decoder import Stage1Decoder
from .encoder import Stage1Encoder
from . import first_stage
from .first_stage import ClassMeter, Stage1Autoencoder, class_loss_sums, class_losses
from .latent_si import LatentSIV3
from .losses import Loss, geom_loss_sums, geom_losses
from .metrics import DisplacementErrors, DisplacementMeter, displacement_errors, displacement_rows
from .peptide_loss import PeptideLoss, peptide_loss_sums, peptide_losses
from .sampling import (RolloutSampler, SecondStageSampler, best_of_k_errors, min_ade_fde, sample_rollout, sample_sharded,
                       setup_conditioning, shard_bounds)
from . import kmeans, tica
from .kmeans import KMeansResult, kmeans_fit, nearest_rows
from .tica import (TicaHistograms, TicaModel, assign_centers, cossin_features, fit_microstates, lagged_moments, linspace_edges, metastable_jsd, solve_tica,
                   tica_autocovariance, tica_covariances, tica_dimension, tica_histograms, tica_jsd, transition_counts)
from .torsion_stats import (TorsionStats, angle_histograms, decorrelation, dihedral_angles, eval_torsion_quads, js_distance, lagged_products,
                            summary_metrics, topology_atoms)
from . import msm
from .msm import MarkovModel, active_set, estimate_markov_model, markov_state_block, pcca_assignments
from . import structure_stats
from .structure_stats import (CaFrameStats, StructureTables, backbone_torsion_quads, ca_atoms, ca_frame_stats, ca_pair_table, column_edges, density_js,
                              histogram_columns, joint_density_js, js_distance_density, pair_distances, tica_atom_selection, tica_features,
                              traj_analysis, triu_pairs)
from . import koopman_tica
from .koopman_tica import KoopmanWeights, WideTicaModel, koopman_weights, run_tica, weighted_moments
from . import superpose
from .superpose import center_coordinates, create_trajectory, rmsd, rmsf, superpose_atom14
from .transport import (CreateTransport, ModelType, PathType, Sampler, SampleResult, Transport, WeightType, as_transport, device_randn,
                        dot_rows, mix_seed, si_reduce)

__all__ = ["msm", "MarkovModel", "active_set", "estimate_markov_model", "markov_state_block", "pcca_assignments", "koopman_tica", "KoopmanWeights", "WideTicaModel", "koopman_weights", "run_tica", "weighted_moments", "LatentSIV3", "CreateTransport", "Transport", "Sampler", "SampleResult", "ModelType", "PathType", "WeightType",
           "SecondStageSampler", "setup_conditioning", "sample_sharded", "shard_bounds", "min_ade_fde", "sample_rollout", "best_of_k_errors",
           "RolloutSampler", "Stage1Decoder", "Stage1Encoder", "as_transport", "device_randn", "dot_rows", "mix_seed", "si_reduce", "Loss", "geom_losses", "geom_loss_sums", "PeptideLoss", "peptide_losses", "peptide_loss_sums", "displacement_rows", "displacement_errors",
           "DisplacementErrors", "DisplacementMeter", "TorsionStats", "dihedral_angles", "angle_histograms", "js_distance", "lagged_products",
           "decorrelation", "eval_torsion_quads", "topology_atoms", "summary_metrics", "tica", "TicaModel", "TicaHistograms", "cossin_features",
           "lagged_moments", "tica_covariances", "solve_tica", "tica_dimension", "linspace_edges", "tica_histograms", "tica_jsd", "assign_centers",
           "transition_counts", "metastable_jsd", "tica_autocovariance", "kmeans", "kmeans_fit", "nearest_rows", "KMeansResult", "fit_microstates", "install", "uninstall", "dropin", "_lib",
           "structure_stats", "traj_analysis", "StructureTables", "CaFrameStats", "pair_distances", "ca_frame_stats", "tica_features", "column_edges",
           "histogram_columns", "js_distance_density", "density_js", "joint_density_js", "ca_atoms", "ca_pair_table", "backbone_torsion_quads",
           "tica_atom_selection", "triu_pairs",
           "superpose", "center_coordinates", "create_trajectory", "rmsd", "rmsf", "superpose_atom14",
           "first_stage", "Stage1Autoencoder", "ClassMeter", "class_losses", "class_loss_sums"]
