"""nnmnkwii_amd -- MI355X-native MLPG parameter generation and DTW alignment
behind the Python signatures of r9y9/nnmnkwii's hot path.

    nnmnkwii_amd.paramgen       mlpg, mlpg_grad, unit_variance_mlpg_matrix, reshape_means, ...;
                                gv, gv_stats, mlpg_gv, mlpg_gv_batch (MLPG with the likelihood of the trajectory's gv)
    nnmnkwii_amd.autograd       mlpg / MLPG, unit_variance_mlpg / UnitVarianceMLPG (torch, ROCm)
    nnmnkwii_amd.preprocessing  trim_zeros_frames, delta_features, alignment.DTWAligner / IterativeDTWAligner,
                                modspec / inv_modspec / modspec_smoothing / modspec_smoothing_batch
    nnmnkwii_amd.baseline.gmm   MLPGBase, MLPG (GMM voice-conversion baseline; caller of paramgen.mlpg; MLPG(..., gv=...) adds the gv stage)
    nnmnkwii_amd.postfilters    merlin_post_filter, merlin_post_filter_batch (mel-cepstral post-filter behind MLPG),
                                modspec_post_filter, modspec_post_filter_batch, modspec_log_stats, modspec_post_filter_tables
                                (modulation-spectrum post-filter)
    nnmnkwii_amd.mixture        fit_gaussian_mixture, predict_proba, predict, score_samples (full-covariance GMM, float64 EM)
    nnmnkwii_amd.metrics        melcd, mean_squared_error, lf0_mean_squared_error, vuv_error; batch_metrics (several of them over one
                                padded batch in one call).  Host arrays are evaluated on the host, CUDA tensors on the device.
    nnmnkwii_amd.preprocessing.f0  interp1d, interp1d_batch (the unvoiced gaps of F0 tracks filled, and the V/UV flag, over padded
                                batches; also exported from nnmnkwii_amd.preprocessing)
    nnmnkwii_amd.preprocessing.wave  mulaw, inv_mulaw, mulaw_quantize, inv_mulaw_quantize, preemphasis, inv_preemphasis;
                                wave_encode_batch, wave_decode_batch (waveform crops to classes and generated classes to waveforms
                                over padded batches, one launch each; also exported from nnmnkwii_amd.preprocessing)
    nnmnkwii_amd.preprocessing.frames  remove_zeros_frames, remove_zeros_frames_batch, joint_features_batch (the joint rows of a
                                voice-conversion recipe: deltas, concatenation and zero-frame removal in three launches; also exported
                                from nnmnkwii_amd.preprocessing)
    nnmnkwii_amd.frontend.merlin  frame_features, frame_features_batch (phone-level linguistic features and durations to the
                                frame-level input matrix of an acoustic model), get_frame_feature_size, coarse_coding_table;
                                kept_frame_features, kept_frame_features_batch (the same without the frames of silent phones)
    nnmnkwii_amd.preprocessing.silence  remove_silence_frames, remove_silence_frames_batch (the frames of silent phones dropped
                                from any frame-level matrix over padded batches; also exported from nnmnkwii_amd.preprocessing)

Everything numerical runs in hand-written HIP kernels (``csrc/``) behind the
C ABI of ``include/mlpg_hip.h`` (the objective metrics: its extension header
``include/nnmnkwii_metrics.h``; the frontend: ``include/nnmnkwii_frontend.h``; continuous F0: ``include/nnmnkwii_f0.h``; the waveform codec: ``include/nnmnkwii_wave.h``; the joint rows: ``include/nnmnkwii_joint.h``; silence removal: ``include/nnmnkwii_silence.h``).  There is no CPU fallback: without the built
extension or without a GPU the calls raise ``HipExtensionError``.
"""
from ._hip import HipExtensionError  # noqa: F401

__version__ = "0.1.0"
