"""ctypes binding of libwavenet_hip.so (include/wavenet_hip.h).

The HIP library is THE compute path: there is no CPU or PyTorch fallback.
If the shared object is missing or a call fails, this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('WN_LIB_PATH') or os.path.join(
    os.path.dirname(_HERE), 'libwavenet_hip.so')   # WN_LIB_PATH: A/B builds

c_int, c_long, c_float = ctypes.c_int, ctypes.c_long, ctypes.c_float
c_double = ctypes.c_double
c_void_p, c_u64 = ctypes.c_void_p, ctypes.c_uint64
P = c_void_p  # every device / host pointer crosses as a raw address

# name -> (restype, argtypes); mirrors include/wavenet_hip.h one to one
SIGNATURES = {
    'wn_version': (c_int, []),
    'wn_error_string': (ctypes.c_char_p, [c_int]),
    'wn_mu_law_thresholds_host': (c_int, [c_int, P]),
    'wn_mu_law_decode_table_host': (c_int, [c_int, P]),
    'wn_mu_law_encode': (c_int, [P, P, c_long, P, c_int, P]),
    'wn_mu_law_decode': (c_int, [P, P, c_long, P, c_int, P]),
    # input noise: [audio,] codes, codes_in, keys, lengths, B, T, [thr,] Q,
    # seed, thresh, width, stream
    'wn_code_noise': (c_int, [P, P, P, P, c_int, c_int, c_int, c_u64, c_int,
                              c_int, P]),
    'wn_mu_law_encode_noisy': (c_int, [P, P, P, P, P, c_int, c_int, P, c_int,
                                       c_u64, c_int, c_int, P]),
    'wn_causal_gather': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int,
                                 P]),
    'wn_scalar_causal_fwd': (c_int, [P, P, c_int, P, c_int, c_int, c_int, P]),
    'wn_scalar_causal_wgrad': (c_int, [P, P, P, c_int, c_int, c_int, c_int,
                                       P]),
    'wn_causal_wgrad_slabs': (c_int, [c_long]),
    'wn_causal_wgrad': (c_int, [P, P, P, c_int, c_int, c_int, c_int, P]),
    'wn_layer_fwd': (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int,
                             c_int, c_int, P]),
    'wn_stack_flag_count': (c_long, [c_int, c_int, c_int]),
    'wn_stack_wimg_floats': (c_int, []),
    'wn_stack_tile_rows': (c_int, [c_int, c_int, c_int]),
    'wn_stack_pack': (c_int, [P, c_long, P, P, c_int, P]),
    'wn_stack_fwd': (c_int, [P, P, P, P, P, c_long, c_int, P, P, P, P,
                             c_int, c_int, c_int, c_int, c_int, P]),
    'wn_stack_fwd_skip': (c_int, [P, P, P, P, P, c_long, c_int, P, P, P, P,
                                  c_int, c_int, c_int, c_int, c_int, P, P, P, P]),
    'wn_stack_fwd_skip_ok': (c_int, [c_int, c_int, c_int, c_int]),
    'wn_stack_skip_img_floats': (c_long, [c_int]),
    'wn_stack_skip_pack': (c_int, [P, c_int, P, P]),
    'wn_stack_fwd_lc': (c_int, [P, P, P, P, P, c_long, c_int, P, P, P, P,
                                c_int, c_int, c_int, c_int, c_int, P, c_long,
                                P]),
    'wn_stack_bwd_slabs': (c_int, [c_int, c_int, c_int]),
    'wn_stack_fwd_waves': (c_int, [c_int, c_int, c_int]),
    'wn_stack_bwd_waves': (c_int, [c_int, c_int, c_int, P]),
    'wn_stack_bwd': (c_int, [P, P, P, P, P, c_long, P, P, P, c_long, P, P, P,
                             P, P, c_int, c_int, c_int, c_int, P]),
    'wn_stack_bwd_lc': (c_int, [P, P, P, P, P, c_long, P, P, P, c_long, P, P,
                                P, P, P, c_int, c_int, c_int, c_int, P, c_long,
                                P]),
    'wn_layer_wgrad_slab_floats': (c_int, []),
    'wn_dense_planes': (c_int, [P, c_long, P, P, P, c_long, P, c_long, c_long, c_int,
                                P]),
    'wn_dense_planes_gate': (c_int, [P, c_long, P, P, c_long, P, P, c_long, P, P,
                                     c_long, c_long, c_int, P]),
    'wn_layer_fwd_k': (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_int, P]),
    'wn_layer_bwd_k': (c_int, [P, P, P, P, P, P, P, P, P, P, P, c_int, c_int,
                               c_int, c_int, c_int, c_int, c_int, c_long, P]),
    'wn_layer_wgrad_k': (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int,
                                 c_int, c_int, c_int, c_int, c_long, P]),
    'wn_layer_fwd_blk': (c_int, [P, c_long, c_int, P, P, P, P, P, c_int, P, P,
                                 c_int, c_int, c_int, c_int, c_int, c_int,
                                 c_int, P, P, c_long, c_int, c_int, c_int,
                                 c_long, P]),
    'wn_layer_bwd_blk': (c_int, [P, P, c_long, c_int, P, P, P, P, c_int,
                                 c_long, c_int, c_int, c_int, c_int, c_int,
                                 c_int, c_int, c_long, P]),
    'wn_layer_bwd2_slabs': (c_int, [c_int, c_int]),
    'wn_layer_bwd2_wimg_floats': (c_int, []),
    'wn_layer_bwd2_pack': (c_int, [P, c_long, P, c_int, P]),
    'wn_layer_bwd2': (c_int, [P, P, P, P, P, P, P, P, P, P, c_int, c_int,
                              c_int, P]),
    'wn_gemm_nn': (c_int, [P, c_long, c_int, c_long, P, c_int, P, P, c_long,
                           P, c_long, P, c_long, c_int, c_long, P, c_long,
                           c_int, c_int, c_int, P]),
    'wn_gemm_split_w_bytes': (c_long, [c_int, c_int]),
    'wn_gemm_nn_split': (c_int, [P, c_long, c_int, c_long, P, c_int, P, P,
                                 c_long, P, c_long, P, c_long, c_int, c_long,
                                 P, c_long, c_int, c_int, c_int, P, c_int, P]),
    'wn_gemm_tn_tail_rows': (c_int, [c_int, c_int]),
    'wn_gemm_tn_slab_floats': (c_long, [c_int, c_int]),
    'wn_gemm_tn_splits': (c_int, [c_long, c_int, c_int, c_int]),
    'wn_gemm_tn_split': (c_int, [P, c_long, c_int, c_long, P, c_long, P, c_int,
                                 c_long, c_int, c_int, c_int, c_int, P]),
    'wn_gemm_tn': (c_int, [P, c_long, c_int, c_long, P, c_int, c_int, P,
                           c_long, P, c_int, c_long, c_int, c_int, c_int, P]),
    'wn_reduce_slabs': (c_int, [P, c_int, c_long, c_int, c_long, c_long,
                                c_long, P, c_long, c_int, c_long, P]),
    'wn_reduce_slabs_mt': (c_int, [P, c_int, c_long, c_long, P, c_long, P, c_int,
                                   c_long, c_int, P]),
    'wn_reduce_pair_slabs': (c_int, [P, c_int, c_int, c_int, c_int, c_int, P,
                                     c_int, c_long, c_int, c_int, P]),
    'wn_transpose': (c_int, [P, c_int, c_int, c_long, P, c_long, P]),
    'wn_xent_partials': (c_int, [c_long]),
    'wn_xent': (c_int, [P, c_long, P, P, P, c_int, c_int, c_int, c_int, P]),
    'wn_xent_masked': (c_int, [P, c_long, P, P, P, P, P, c_int, c_int, c_int,
                               c_int, P]),
    # logits, ld, q, starts, lengths, inv_den, dlogits, loss_partials, B, T,
    # Q, tf_quirk, stream
    'wn_xent_window': (c_int, [P, c_long, P, P, P, P, P, P, c_int, c_int,
                               c_int, c_int, P]),
    # (wn_xent_score's arguments with starts in front of lengths)
    'wn_xent_score_window': (c_int, [P, c_long, P, P, P, P, P, P, P, P, c_int,
                                     c_int, c_int, P]),
    # logits, ld, q, lengths, row_nll, clip_nll, clip_count, clip_correct,
    # scratch, B, T, Q, stream
    'wn_xent_score_scratch_floats': (c_long, [c_long]),
    'wn_xent_score': (c_int, [P, c_long, P, P, P, P, P, P, P, c_int, c_int,
                              c_int, P]),
    'wn_softmax64_row': (c_int, [P, c_int, P, P]),
    'wn_adam': (c_int, [P, P, P, P, c_long, c_float, c_float, c_float,
                        c_float, c_float, c_float, P, P]),
    'wn_momentum': (c_int, [P, P, P, c_long, c_float, c_float, c_float,
                            c_float, P, P]),
    'wn_rmsprop': (c_int, [P, P, P, P, c_long, c_float, c_float, c_float,
                           c_float, c_float, c_float, P, P]),
    # the updates behind a global-norm clip, with EMA shadow weights:
    # ..., partials, nparts, clip_norm, ema, ema_decay, norm_out, stream
    'wn_grad_norm_partials_count': (c_int, []),
    'wn_grad_norm_partials': (c_int, [P, c_long, P, P]),
    'wn_adam_clip': (c_int, [P, P, P, P, c_long, c_float, c_float, c_float,
                             c_float, c_float, c_float, P, P, c_int, c_float,
                             P, c_float, P, P]),
    'wn_momentum_clip': (c_int, [P, P, P, c_long, c_float, c_float, c_float,
                                 c_float, P, P, c_int, c_float, P, c_float, P,
                                 P]),
    'wn_rmsprop_clip': (c_int, [P, P, P, P, c_long, c_float, c_float, c_float,
                                c_float, c_float, c_float, P, P, c_int,
                                c_float, P, c_float, P, P]),
    'wn_l2_partials_count': (c_int, []),
    'wn_l2_partials': (c_int, [P, c_long, P, P, P]),
    'wn_gc_bias': (c_int, [P, c_long, c_long, c_long, c_int, P, c_int, P, P,
                           c_int, c_int, c_int, P]),
    'wn_colsum_clip_chunks': (c_int, [c_int]),
    'wn_colsum_clip': (c_int, [P, P, c_int, c_int, P, P, P]),
    'wn_gc_grad': (c_int, [P, c_long, c_long, c_int, P, c_int, P, P, c_int,
                           c_int, P, P, P, c_int, P]),
    'wn_causal_conv': (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_int,
                               c_int, P]),
    'wn_time_to_batch': (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    'wn_batch_to_time': (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    'wn_diag_mfma_peak': (c_int, [P, c_int, c_int, P]),
    'wn_axpy': (c_int, [P, P, c_float, P, c_long, P]),
    'wn_fill': (c_int, [P, c_long, c_float, P]),
    'wn_sum_rows': (c_int, [P, c_int, c_int, P, P]),
    'wn_fastgen_state_floats': (c_long, [P, c_int]),
    'wn_fastgen_init': (c_int, [P, c_long, P, c_int, P]),
    'wn_fastgen_run': (c_int, [P, P, c_long, P, P, P, P, P, P, P, P, c_int,
                               c_int, c_int, P, P, P, c_int, c_int, c_float,
                               c_u64, P, c_int, c_int, c_int, P]),
    'wn_fastgen_run_wide': (c_int, [P, P, c_long, P, P, P, P, P, P, P, P,
                                    c_int, c_int, c_int, c_int, P, P, P, c_int,
                                    c_int, c_float, c_u64, P, c_int, c_int,
                                    c_int, P, P]),
    'wn_fastgen_wide_coop_bytes': (c_long, [c_int, c_int, c_int, c_int]),
    'wn_fastgen_step': (c_int, [P, P, c_long, P, P, P, P, P, P, P, P, c_int,
                                c_int, c_int, P, P, P, P, P, c_int, P, P, P,
                                P, P, P, P]),
    'wn_fastgen_persist_workgroups': (c_int, [c_int, c_int, c_int]),
    'wn_fastgen_persist_role': (c_int, [c_int, c_int, c_int]),
    'wn_fastgen_persist_ll_words': (c_long, [c_int, c_int, c_int]),
    'wn_fastgen_persist': (c_int, [P, P, c_long, P, P, P, P, P, P, P, P, c_int,
                                   c_int, c_int, P, P, P, P, P, c_int, P, P, P,
                                   P, P, P, P, P, c_int, P]),
    'wn_fastgen_pre': (c_int, [P, c_long, P, P, c_int, P, P, P, P]),
    'wn_fastgen_finish': (c_int, [c_int, P, P, P, P, P, P]),
    'wn_fastgen_pack': (c_int, [P, c_long, P, c_int, P]),
    'wn_fastgen_batch_rows': (c_int, [c_int]),
    'wn_fastgen_batch_state_floats': (c_long, [P, c_int, c_int]),
    'wn_fastgen_batch_init': (c_int, [P, c_long, P, P, c_int, P]),
    'wn_fastgen_batch_pre': (c_int, [P, c_long, P, c_int, P, c_int, c_int, P,
                                     P, P, P]),
    'wn_fastgen_batch_step': (c_int, [P, P, c_long, P, P, P, P, P, P, P,
                                      c_int, P, c_int, c_int, c_int, c_int, P,
                                      P, P, P, P, P, P, c_int, P, P, P, P, P,
                                      P]),
    'wn_fastgen_batch_stages': (c_int, [c_int, c_int, P, P, c_long, P, P, P,
                                        P, P, P, P, c_int, P, c_int, c_int,
                                        c_int, c_int, P, P, P, P, P, P, P,
                                        c_int, P, P, P, P, P, P]),
    'wn_fastgen_batch_finish': (c_int, [c_int, c_int, P, P, P, P, P, P, P]),
    # local conditioning: the conditioned-bias ring and the _lc variants
    # (the entry point's arguments + ring, its rows R, its stream stride)
    'wn_fastgen_lc_bias': (c_int, [P, c_long, c_int, P, c_int, P, c_int,
                                   c_int, c_long, c_int, P, c_int, c_int, P]),
    # learned upsampling of frame-rate LC features (the scales: a host array)
    'wn_lc_upsample_floats': (c_int, [P, c_int, c_int]),
    'wn_lc_upsample_fwd': (c_int, [P, c_int, P, P, P, c_int, c_int, c_int, P,
                                   c_int, c_int, c_int, P]),
    'wn_lc_upsample_bwd_slabs': (c_int, [c_long, c_int]),
    'wn_lc_upsample_bwd': (c_int, [P, c_int, P, P, P, c_int, c_int, c_int, P,
                                   c_int, c_int, c_int, P, c_int, c_long, P]),
    'wn_lc_upsample_bwd_ctx': (c_int, [P, c_int, P, P, P, c_int, c_int, c_int,
                                       P, c_int, c_int, c_int, P, c_int,
                                       c_long, P, P, P]),
    # frame-context convolution in front of the upsampler
    'wn_lc_context_fwd': (c_int, [P, c_int, P, c_int, c_int, P, c_int, c_int,
                                  P]),
    'wn_lc_context_wgrad_slabs': (c_int, [c_long, c_int]),
    'wn_lc_context_wgrad': (c_int, [P, c_int, P, c_int, c_int, c_int, c_int, P,
                                    c_int, c_long, P]),
    # log-mel front end: audio, ld, B, T, lengths, window, basis, melw, n_fft,
    # hop, n_bins, n_mels, floor, out, stream
    'wn_melspec': (c_int, [P, c_long, c_int, c_int, P, P, P, P, c_int, c_int,
                           c_int, c_int, c_float, P, P]),
    # feature normalisation.  stats: fr, B, F, C, nframes, acc, partials,
    # stream; normalize: in, out, B, F, C, nframes, shift, scale, lo, hi, stream
    'wn_feature_stats_partials_count': (c_int, []),
    'wn_feature_stats': (c_int, [P, c_int, c_int, c_int, P, P, P, P]),
    'wn_feature_normalize': (c_int, [P, P, c_int, c_int, c_int, P, P, P,
                                     c_float, c_float, P]),
    # distance of two feature tensors: a, b, B, F, C, nframes, abs_sum,
    # sq_sum, rms_sum, partials, stream
    'wn_feature_distance_partials': (c_long, [c_int, c_int]),
    'wn_feature_distance': (c_int, [P, P, c_int, c_int, c_int, P, P, P, P, P,
                                    P]),
    # pre- / de-emphasis: in, out, ld_in, ld_out, B, T, lengths, [initial,
    # last,] alpha, stream
    'wn_emphasis_chunk': (c_int, []),
    'wn_preemphasis': (c_int, [P, P, c_long, c_long, c_int, c_int, P, c_float,
                               P]),
    'wn_deemphasis': (c_int, [P, P, c_long, c_long, c_int, c_int, P, P, P,
                              c_float, P]),
    # device-resident corpus.  The plan (13 arguments): utt_off, utt_len, U,
    # item_utt, item_start, P, perm, e0, nE, g0, size, random, seed.
    # gather: flat, N, plan, audio, B, T, stream
    'wn_corpus_window_frames': (c_long, [c_int, c_int, c_int]),
    'wn_corpus_gather': (c_int, [P, c_long, P, P, c_int, P, P, c_int, P,
                                 c_long, c_int, c_long, c_int, c_int, c_u64,
                                 P, c_int, c_int, P]),
    # frames, NF, fr_off, fr_len, plan, hop, ctx, Lc, frames, Fw, rows, B, T,
    # stream
    'wn_corpus_gather_frames': (c_int, [P, c_long, P, P, P, P, c_int, P, P,
                                        c_int, P, c_long, c_int, c_long,
                                        c_int, c_int, c_u64, c_int, c_int,
                                        c_int, P, c_int, P, c_int, c_int, P]),
    # (the two above with `history` behind seed; wn_corpus_gather_hist: and
    # hist, lens behind audio)
    'wn_corpus_gather_hist': (c_int, [P, c_long, P, P, c_int, P, P, c_int, P,
                                      c_long, c_int, c_long, c_int, c_int,
                                      c_u64, c_int, P, P, P, c_int, c_int,
                                      P]),
    'wn_corpus_gather_frames_hist': (c_int, [P, c_long, P, P, P, P, c_int, P,
                                             P, c_int, P, c_long, c_int,
                                             c_long, c_int, c_int, c_u64,
                                             c_int, c_int, c_int, c_int, P,
                                             c_int, P, c_int, c_int, P]),
}
for _name in ('wn_fastgen_run', 'wn_fastgen_pre', 'wn_fastgen_step',
              'wn_fastgen_persist', 'wn_fastgen_batch_pre',
              'wn_fastgen_batch_step'):
    # ..., const float* lc_ring, int lc_R, int lc_stride, void* stream
    _res, _args = SIGNATURES[_name]
    SIGNATURES[_name + '_lc'] = (_res, _args[:-1] + [P, c_int, c_int, P])
for _name in ('wn_fastgen_run', 'wn_fastgen_run_wide', 'wn_fastgen_run_lc'):
    # ..., int top_k, float top_p, void* stream (the truncated draw; 0: off)
    _res, _args = SIGNATURES[_name]
    SIGNATURES[_name + '_trunc'] = (_res, _args[:-1] + [c_int, c_float, P])
for _name in ('wn_fastgen_batch_step', 'wn_fastgen_batch_step_lc',
              'wn_fastgen_batch_finish'):
    # ..., const int32_t* origins, void* stream (restarted streams: the draw
    # counted from each stream's own origin)
    _res, _args = SIGNATURES[_name]
    SIGNATURES[_name + '_q'] = (_res, _args[:-1] + [P, P])
# state, dilations, L, B, cursors, prev, origins, flags, stream
SIGNATURES['wn_fastgen_batch_restart'] = (c_int, [P, P, c_int, c_int, P, P, P,
                                                  P, P])
# table, B, n, Lc, pos0, out, stream
SIGNATURES['wn_fastgen_batch_lc_rows'] = (c_int, [P, c_int, c_int, c_int,
                                                  c_long, P, P])

# name -> (restype, argtypes); mirrors include/wavenet_pitch.h one to one (the
# pitch tracker's header, bound onto the same library)
PITCH_SIGNATURES = {
    'wn_pitch_tau_min': (c_int, [c_float, c_float]),
    'wn_pitch_tau_max': (c_int, [c_float, c_float]),
    'wn_pitch_lds_bytes': (c_long, [c_int, c_int, c_int]),
    # audio, lengths, ld, B, T, hop, window, tau_min, tau_max, threshold,
    # silence, sample_rate, f0, aper, lag, cmnd, stream
    'wn_pitch_track': (c_int, [P, P, c_long, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_float, c_float, c_float, P, P, P, P,
                               P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_pitch_path.h one to one
# (the pitch path's header, bound onto the same library)
PITCH_PATH_SIGNATURES = {
    'wn_pitch_path_workspace_bytes': (c_long, [c_int, c_int, c_int, c_int]),
    # cmnd, lag_in, nframes, B, F, tau_min, tau_max, pen, bias, switch_cost,
    # unvoiced_cost, sample_rate, workspace, f0, aper, lag, cost, stream
    'wn_pitch_path': (c_int, [P, P, P, c_int, c_int, c_int, c_int, P, P,
                              c_float, c_float, c_float, P, P, P, P, P, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_lc_frames.h one to one
# (the conditioning-frame assembler's header, bound onto the same library)
LC_FRAMES_SIGNATURES = {
    'wn_lc_frames_chunk': (c_int, []),
    # mel, ld_mel, M, shift, scale, lo, hi, f0, mode, fmin, span, nframes, B,
    # F, out, ld_out, c0, stream
    'wn_lc_frames': (c_int, [P, c_long, c_int, P, P, c_float, c_float, P,
                             c_int, c_double, c_double, P, c_int, c_int, P,
                             c_long, c_int, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_spectral.h one to one
# (the synthesis metrics' header, bound onto the same library)
SPECTRAL_SIGNATURES = {
    'wn_stft_distance_partials': (c_long, [c_int, c_int, c_int]),
    'wn_stft_distance_staged': (c_int, [c_int, c_int]),
    # gen, ld_gen, org, ld_org, B, T, lengths, window, basis, n_fft, hop,
    # n_bins, floor, sc_num, sc_den, log_sum, partials, stream
    'wn_stft_distance': (c_int, [P, c_long, P, c_long, c_int, c_int, P, P, P,
                                 c_int, c_int, c_int, c_float, P, P, P, P, P]),
    'wn_cepstral_distance_partials': (c_long, [c_int, c_int]),
    # a, b, B, F, C, nframes, dct, K, mcd_sum, partials, stream
    'wn_cepstral_distance': (c_int, [P, P, c_int, c_int, c_int, P, P, c_int,
                                     P, P, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_griffin_lim.h one to one
# (the Griffin-Lim baseline's header, bound onto the same library)
GRIFFIN_LIM_SIGNATURES = {
    # x, ld_x, B, T, lengths, window, basis, n_fft, hop, n_bins, out, stream
    'wn_stft': (c_int, [P, c_long, c_int, c_int, P, P, P, c_int, c_int, c_int,
                        P, P]),
    'wn_istft_scratch_bytes': (c_long, [c_int, c_int, c_int, c_int]),
    # spec, B, T, lengths, window, basis, n_fft, hop, n_bins, scratch, x,
    # ld_x, stream
    'wn_istft': (c_int, [P, c_int, c_int, P, P, P, c_int, c_int, c_int, P, P,
                         c_long, P]),
    # frames, B, F, n_mels, nframes, pinv, n_bins, out, stream
    'wn_mel_to_magnitude': (c_int, [P, c_int, c_int, c_int, P, P, c_int, P,
                                    P]),
    # A, B, F, n_bins, keys, seed, mode, tab, c0, stream
    'wn_gl_init': (c_int, [P, c_int, c_int, c_int, P, c_u64, c_int,
                           P, P, P]),
    'wn_gl_project_partials': (c_long, [c_int, c_int, c_int]),
    # x, ld_x, B, T, lengths, window, basis, n_fft, hop, n_bins, A, t_prev,
    # alpha, t_out, c_out, trace, partials, stream
    'wn_gl_project': (c_int, [P, c_long, c_int, c_int, P, P, P, c_int, c_int,
                              c_int, P, P, c_float, P, P, P, P, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_lpc.h one to one
# (linear prediction's header, bound onto the same library)
LPC_SIGNATURES = {
    # frames, B, F, n_mels, nframes, pinv, n_bins, ctab, lagwin, order, out,
    # stream
    'wn_lpc_from_mel': (c_int, [P, c_int, c_int, c_int, P, P, c_int, P, P,
                                c_int, P, P]),
    'wn_lpc_analysis_tile': (c_int, []),
    # in, ld_in, coeffs, F, order, hop, lengths, B, T, gain (synthesis: its
    # inverse), out, ld_out, stream
    'wn_lpc_analysis': (c_int, [P, c_long, P, c_int, c_int, c_int, P, c_int,
                                c_int, c_float, P, c_long, P]),
    'wn_lpc_synthesis': (c_int, [P, c_long, P, c_int, c_int, c_int, P, c_int,
                                 c_int, c_float, P, c_long, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_resample.h one to one
# (the sample-rate converter's header, bound onto the same library)
RESAMPLE_SIGNATURES = {
    'wn_resample_tile': (c_int, []),
    # x, ld_x, lengths, B, T, up, down, Hh, tab, out, ld_out, stream
    'wn_resample': (c_int, [P, c_long, P, c_int, c_int, c_int, c_int, c_int,
                            P, P, c_long, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_stoi.h one to one
# (STOI / ESTOI's header, bound onto the same library)
STOI_SIGNATURES = {
    'wn_stoi_band_edge': (c_int, [c_int]),
    'wn_stoi_scratch_bytes': (c_long, [c_int, c_int]),
    # gen, ld_gen, org, ld_org, lengths, B, T, window, basis, scratch,
    # stoi_sum, estoi_sum, segments, kept, stream
    'wn_stoi': (c_int, [P, c_long, P, c_long, P, c_int, c_int, P, P, P, P, P,
                        P, P, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_mol.h one to one
# (the mixture-of-logistics head's header, bound onto the same library)
MOL_SIGNATURES = {
    # audio, lengths, levels_out, centres_out, B, T, stream
    'wn_mol_quantize': (c_int, [P, P, P, P, c_int, c_int, P]),
    # logits, ld, levels, starts, lengths, inv_den, dlogits, loss_partials,
    # B, T, K, log_scale_min, stream
    'wn_mol_loss': (c_int, [P, c_long, P, P, P, P, P, P, c_int, c_int, c_int,
                            c_float, P]),
    'wn_mol_score_scratch_floats': (c_long, [c_long]),
    # logits, ld, levels, starts, lengths, row_nll, clip_nll, clip_count,
    # scratch, B, T, K, log_scale_min, stream
    'wn_mol_score': (c_int, [P, c_long, P, P, P, P, P, P, P, c_int, c_int,
                             c_int, c_float, P]),
    # logits_row, K, log_scale_min, out, stream
    'wn_mol_params_row': (c_int, [P, c_int, c_float, P, P]),
    # params, seeds, counters, temperature, levels_out, centres_out, R, K,
    # stream
    'wn_mol_sample': (c_int, [P, P, P, c_float, P, P, c_int, c_int, P]),
}

# name -> (restype, argtypes); mirrors include/wavenet_fastgen_mol.h one to one
# (batched fast generation for mixture models, bound onto the same library)
FASTGEN_MOL_SIGNATURES = {
    # state, state_floats, cursors, hist, B, stream
    'wn_fastgen_mol_init': (c_int, [P, c_long, P, P, c_int, P]),
    # wn_fastgen_batch_pre's arguments, lc_ring, lc_R, lc_stride, stream
    'wn_fastgen_mol_pre': (c_int, [P, c_long, P, c_int, P, c_int, c_int, P, P,
                                   P, P, c_int, c_int, P]),
    # causal, K0, layer0, layer_stride, skip_w, skip_bsum, post1_w, post1_b,
    # post2_w, post2_b, gc_bias_fg, bias_stream_stride, dilations, L, S, K, B,
    # state, cursors, hist, samples_io, ctl, seeds, params_out, use_biases,
    # log_scale_min, pre, z_all, h1, h2, logits, lc_ring, lc_R, lc_stride,
    # origins, stream
    'wn_fastgen_mol_step': (c_int, [P, c_int, P, c_long, P, P, P, P, P, P, P,
                                    c_int, P, c_int, c_int, c_int, c_int, P,
                                    P, P, P, P, P, P, c_int, c_float, P, P, P,
                                    P, P, P, c_int, c_int, P, P]),
    # K, log_scale_min, B, cursors, samples_io, ctl, seeds, params_out,
    # logits, origins, stream
    'wn_fastgen_mol_finish': (c_int, [c_int, c_float, c_int, P, P, P, P, P, P,
                                      P, P]),
    # state, dilations, L, B, cursors, hist, origins, flags, stream
    'wn_fastgen_mol_restart': (c_int, [P, P, c_int, c_int, P, P, P, P, P]),
}


_lib = None


class WaveNetHipError(RuntimeError):
    pass


def load():
    """Load the HIP library (once).  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WaveNetHipError(
            'libwavenet_hip.so not found at %s: build it with '
            '`python __graft_entry__.py build` (hipcc --offload-arch=gfx950). '
            'There is no CPU fallback.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for table in (SIGNATURES, PITCH_SIGNATURES, PITCH_PATH_SIGNATURES,
                  LC_FRAMES_SIGNATURES, SPECTRAL_SIGNATURES,
                  GRIFFIN_LIM_SIGNATURES, LPC_SIGNATURES,
                  RESAMPLE_SIGNATURES, STOI_SIGNATURES, MOL_SIGNATURES,
                  FASTGEN_MOL_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def check(code, what=''):
    if code != 0:
        lib = load()
        msg = lib.wn_error_string(int(code)).decode()
        raise WaveNetHipError('%s failed: %s (code %d)' % (what, msg, code))


# ---- launch plans --------------------------------------------------------
# A training step is ~235 kernel launches whose arguments (raw device
# addresses and ints) do not change from step to step.  Re-deriving them in
# Python every step (tensor views, data_ptr(), current_stream()) costs about as
# much host time as the GPU needs for the step, so the host records the
# (function, args) sequence once per workspace and replays it.
_rec = None


class record(object):
    """Context manager: every `call` inside is executed AND appended to
    `self.plan` as (ctypes function, args, name, flops-or-None)."""

    def __enter__(self):
        global _rec
        self._outer = _rec
        self.plan = []
        _rec = self.plan
        return self

    def __exit__(self, *exc):
        global _rec
        _rec = self._outer
        return False


def call(name, *args):
    """Call an int-returning entry point and raise on a non-zero code."""
    lib = load()
    fn = getattr(lib, name)
    if _rec is not None:
        _rec.append((fn, args, name, None))
    code = fn(*args)
    if code != 0:
        check(code, name)


def call_py(fn):
    """Run a host-side action that belongs INTO the launch sequence (a
    cross-stream event record / wait) and, while recording, append it to the
    plan so that a replay repeats it at the same position."""
    def wrapped():
        fn()
        return 0
    if _rec is not None:
        _rec.append((wrapped, (), 'py', None))
    wrapped()


def call_timed(name, args, flops, events):
    """`call` for the GEMMs; with `events` (a list) the launch is bracketed by
    HIP events on torch's current stream and (start, end, flops) is appended
    (bench.py's live roofline measurement)."""
    lib = load()
    fn = getattr(lib, name)
    if _rec is not None:
        _rec.append((fn, args, name, flops))
    _timed(fn, args, name, flops, events)


def _timed(fn, args, name, flops, events):
    if events is None:
        code = fn(*args)
    else:
        import torch
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        code = fn(*args)
        e.record()
        events.append((s, e, flops, name))
    if code != 0:
        check(code, name)


def replay(plan, events=None):
    for fn, args, name, flops in plan:
        if flops is not None and events is not None:
            _timed(fn, args, name, flops, events)
        else:
            code = fn(*args)
            if code != 0:
                check(code, name)


def ptr(t):
    """Raw address of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stack_variant(rows=0, waves=0):
    """WN_STACK_VARIANT of include/wavenet_hip.h: the explicit variant word of
    the stack launches (0 = the library's choice for the shape)."""
    return (rows & 0x3f) | ((waves & 0xf) << 8)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise WaveNetHipError(
            'no MI355X/ROCm device visible: the wavenet HIP path needs a GPU '
            '(there is no CPU fallback)')
