/* emdenoise_dev.h -- DEVELOPMENT hooks of libemdenoise.so.  NOT part of the drop-in boundary (include/emdenoise.h).
 *
 * These are the only places where the library keeps process-global mutable state.  They default to "off", change
 * speed only (kernel variant selection, in-kernel time stamps), never results beyond what DESIGN.md states for the
 * variant, and exist for the A/B tools under tools/ and for bench.py's isolated-GEMM comparison.  A product host must
 * not call them.  Every symbol the shared library exports with an emd_ prefix is declared either in emdenoise.h or
 * here (tests/test_abi.py checks both directions).
 *
 * Nothing in the library reads the environment.  The kernel-selection knobs are fields of one struct (csrc/emd_common.hpp, emd::Knobs),
 * set by name through emd_debug_knob; defaults = the measured-best path (the sep_* knobs, epi_width and nt_mask bit 1 are read by
 * csrc/sep_entry.hip, which routes the fused separable conv; emd_debug_sep_plan below shows what they choose.  conv3_pipe, deconv_direct,
 * nt_mask bit 0, and epi_width, sep_tpw and sep_ablate for conv3_pipe / deconv_pipe are read by csrc/conv_entry.hip, which routes the
 * dense and transposed convs: emd_debug_conv_plan.  The split_* knobs and nt_mask bit 2 are read by csrc/gemm_split.hip):
 *   sep_pipe (1)        1: the LDS-DMA pipelined fused separable conv (csrc/sep_pipe.hip) where it covers the shape, 0: csrc/sep_fused.hip
 *   sep_pipe2_chunk (-1) two fp32 outputs on the 256-column tile (more than 64 channels in one of them; H % 8 == 0, W % 32 == 0): 1 = the whole-chunk
 *                       instance of csrc/sep_pipe2.hip, 0 = csrc/sep_pipe.hip's lockstep kernel (same bits), -1 = the rule (the faster one)
 *   sep_pipe2 (0)       csrc/sep_pipe2.hip's run-time parity instances: 0 never, 1 two outputs of more than 64 columns, 2 wherever it has an instance
 *   sep_gen_pipe (0)    generated-input fused separable conv: 1 = csrc/sep_pipe.hip's 4-wave instance, 0 = csrc/sep_fused.hip (same bits)
 *   sep_mode (-1)       sep_pipe schedule of the one-output instances: -1 = rule, 0 / 1 = the patch requested two / one steps ahead
 *   sep_nw (0)          sep_pipe waves per workgroup: 0 = rule (4 wherever there is an instance), 8 (8 x 32 pixel tiles, one workgroup per CU)
 *                       or 4 (8 x 16 tiles, two per CU: up to 128 output columns, 64 | 64 for two outputs)
 *   sep_ablate (0)      sep_pipe timing experiments: bit 0 no depthwise stage, 1 no MFMA stage, 2 no epilogue, 3 no patch DMA after the
 *                       prologue, 4 no weight DMA after it, 5 no residual loads -- RESULTS ARE WRONG when non-zero
 *   sep_tpw (0)         tiles per workgroup of the fused separable convs (0 = rule)
 *   sep_xcd (1)         0 = launch-order tiles instead of one contiguous run of tiles per XCD
 *   sep_wide (1)        sep_fused 256-column single-output form: 0 never, 1 Cin <= 256, 2 whenever it fits
 *   sep_wres (1)        0 = per-chunk pointwise weight loads in sep_fused's 64-column instances (default: resident in LDS)
 *   epi_width (0)       epilogue of sep_pipe / conv3_pipe / deconv_pipe: 1 = a lane keeps its channel and stores one dword per pixel, 4 = 4 x 4 transpose
 *                       inside lane quads, then 16 bytes per lane; 0 = the kernel's rule (same values either way)
 *   deconv_direct (3)   one-launch transposed conv: 3 = the patch-resident kernel (csrc/deconv_pipe.hip; sums chunk-major: last-bit
 *                       differences to the GEMM forms) where H % 8 == 0 and W % 32 == 0, else as 1; 1 = GEMM form with the epilogue straight
 *                       from the accumulators; 2 = the same on 128-row tiles, two workgroups per CU; 0 = LDS-staged epilogue
 *   nt_mask (7)         non-temporal output stores: bit 0 split32 convolutions, bit 1 sep_fused, bit 2 pointwise split32 GEMM
 *   dw_xcd (1)          depthwise kernels: 0 = launch-order tiles, 1 = XCD-contiguous up to 128 x 128 maps, 2 = always
 *   dw_th (0)           strip height of the rolling depthwise kernel: 4, 8, 16 or 32 (anything else = rule)
 *   split_narrow (1)    pointwise split32 GEMM: 128 x 64 tiles for the small batches whose 128 x 128 tiles leave CUs idle (0 = never)
 *   conv3_pipe (1)      dense 3x3 conv, stride 1, rate 1, H % 8 == 0, W % 32 == 0, <= 256 output channels (2: any width): the patch-resident kernel
 *                       (conv3_pipe.hip; sums chunk-major, taps inside: last-bit differences to the tap-major GEMM), 0 = gemm_split_conv_kernel
 *   split_wide (0)      pointwise split32 GEMM: 256 x 192 tiles where they fill the chip (N = 728: four column tiles, no half round): 0 never
 *                       (default: same bits, slower inside graph D), 1 = 8 waves of 64 x 96, 2 = 4 waves of 128 x 96
 *   split_variant (-1)  pointwise split32 GEMM pipeline variant (-1 = dispatch rule)
 *   split_lead (2)      pointwise split32 GEMM, 16x16x32 form: the DMA of tile kt + 3 issued in step kt into the stage of tile kt (whose fragments
 *                       are in registers): two tiles in flight on three stages; 1 = one step ahead (round 2's schedule; same bits)
 *   exitwave_composed (0)  emd_exitwave_reconstruct_f64 at pad_periods == 0: 1 = the iteration composed from the launches of
 *                       emd_propagate_f64 (the path of pad_periods > 0) instead of the two-launch frequency-domain iteration; differences
 *                       at rounding level.  emd_exitwave_workspace_bytes follows it: set it before asking for the size
 *   up_fused (1)        graph D's native executor: the 4x upsampling of the ASPP output is formed inside its two consumers
 *                       (emd_conv1x1_up_f32, emd_dw3x3_up_split32_f32) instead of written into the concat buffer; 0 = the resize launch
 *                       (residual2_d's sum is associated differently: rounding-level differences)
 *   resize_generic (0)  emd_resize_f32: 1 = the instance whose one inner loop serves every form, instead of the loops for the fixed
 *                       forms (at most four taps) and for runs (same bits; the A/B of tools/resample_bench.py)
 */
#ifndef EMDENOISE_DEV_H
#define EMDENOISE_DEV_H
#ifdef __cplusplus
extern "C" {
#endif

/* Set one of the knobs above by name.  Returns 0, or -1 for an unknown name. */
int emd_debug_knob(const char* name, long value);
/* Host only, no state: channels per workgroup (16, 4 or 1) of the second stage of a per-channel reduction (bn_stats_final,
 * chan_reduce_final) for `nslab` partials per channel -- the launch rule itself (csrc/emd_common.hpp, emd::reduce_final_cl), so that
 * tests/test_reduce_routes.py can prove which instance each of its shapes selects. */
int emd_debug_reduce_final_cl(int nslab);
/* Host only, no state: 1 where emd_sep3x3_dual_f32 has the whole-chunk instance of csrc/sep_pipe2.hip for the layer's shape (what the knob
 * sep_pipe2_chunk switches; the rule has no batch argument), else 0. */
int emd_debug_sep_pipe2_chunk_covers(int H, int W, int Cin, int Cout, int Cout2);
/* Host only, reads the knobs, touches no device: the plan csrc/sep_entry.hip makes for a fused separable conv of this shape and form --
 * which kernel, on which tiles, with which grid (tests/test_sep_plan.py pins it).  flags: bit 0 REFLECT border, 1 residual, 2 second
 * affine, 3 split32 output, 4 generated input, 5 the same from the image (gen9), 6 generated residual, 7 folded final conv; Cout2 > 0: two
 * outputs.  Returns the route, 0 where no kernel takes the shape (out is then left alone): 1 sep_fused, 2 sep_fused with resident
 * weights, 3 its 256-column form, 4 its two-output form, 5 sep_gen9, 6 sep_pipe, 7 sep_pipe2, 8 sep_pipe2's whole-chunk instance.
 * out = {route, waves per workgroup, tiles per workgroup, grid.x, grid.y, grid.z, sep_pipe schedule, epilogue width (0: sep_fused has
 * one form), xcd, nt}. */
int emd_debug_sep_plan(int B, int H, int W, int Cin, int Cout, int Cout2, int stride, int precision, unsigned flags, int out[10]);
/* Host only, reads the knobs, touches no device: the plan csrc/conv_entry.hip makes for a dense or transposed conv, or a pointwise one
 * on fp32 input -- which kernel, on which tiles, with which grid (tests/test_conv_plan.py pins it).  op: 0 emd_conv1x1_f32 (and its _up /
 * _stats forms), 1 emd_conv3x3_f32, 2 emd_deconv3x3s2_f32, 3 emd_conv1x1_s2_bwd_data_f32, 4 emd_conv3x3_split32_f32,
 * 5 emd_deconv3x3s2_split32_f32, 6 emd_deconv3x3s2_fused_split32_f32.  stride, rate: 1 where the entry has none.  flags: bit 0 residual,
 * 1 second affine, 2 split32 output, 3 statistics, 4 upsampled shift.  ldx, ldy: the pixel pitches in the entry's units, 0 = dense (two
 * routes depend on a pitch: conv3_pipe's 9 * W * ldy < 2^31 and deconv_pipe's 32-bit in-image offsets).  Returns the route, 0 where the
 * entry would answer EMD_E_UNSUPPORTED for the grid or the pitch (out is then left alone): 1 gemm_conv_kernel, 2 its upsampled-shift
 * instance, 3 gemm_split_conv_kernel, 4 conv3_pipe_kernel, 5 gemm_split_conv_kernel<., true>, 6 deconv4_split_kernel,
 * 7 deconv4_half_kernel, 8 deconv_pipe_kernel.  out = {route, tile rows, tile columns, threads per workgroup, grid.x, grid.y, grid.z (of
 * one launch), launches, tiles per workgroup, epilogue width (both 0 but on routes 4 and 8), nt, form}; form: route 1 / 2: 1 = the flat
 * row map; 4 / 8: 1 = split32 output. */
int emd_debug_conv_plan(int op, int B, int H, int W, int Cin, int Cout, int stride, int rate, int precision, unsigned flags, int ldx,
                        int ldy, int out[12]);
/* Force the pipeline variant of emd_conv1x1_split32_f32 (csrc/gemm_split.hip); -1 restores the dispatch rule. */
void emd_debug_split_variant(int v);
/* Host only, reads the knobs and the forced variant, touches no device: what the pointwise split32 GEMM (csrc/gemm_split.hip,
 * emd_conv1x1_split32[_out|_stats|_stats_fold]_f32) launches for M rows -- the function the launcher itself calls (tests/test_split_plan.py
 * pins it).  flags: bit 0 split32 output, bit 1 statistics.  The rule with default knobs, nt = ceil(Cout / 128): 256 x 128 tiles where
 * ceil(M / 256) * nt >= 192 or statistics are asked for; else 128 x 128 where ceil(M / 128) * nt >= 256 or the output is split32; else
 * 128 x 64 (split_narrow).  Returns the kernel id, 0 where nothing would be launched (M < 1, a shape the entry refuses, a grid too
 * large; out is then left alone): 1 gemm_split_kernel<256, 3> (variant 1), 2 <256, 2> (0), 3 gemm_split_persist_kernel (4; weight planes
 * as emd_pack_weights_bf16 lays them, a dense input), 4 <128, 2> (2), 5 gemm_split16_wide_kernel<2> (split_wide 2), 6 <4> (split_wide 1),
 * 7 / 8 / 9 gemm_split16_kernel<128, 64, true> / <128, 128, true> / <256, 128, true> (the default: split_lead 2), 10 / 11 / 12 the same
 * three one step ahead (split_lead 1), 13 gemm_split_kernel<256, 3, true, true> (6), 14 <256, 3, true, false, true> (7),
 * 15 <256, 3, true> (3).  out = {kernel, tile rows, tile columns, threads per workgroup, row tiles, column tiles, split_wide form in use
 * (0: none), K steps ahead (2 or 1 on kernels 7-12, else 0)}; the grid is row tiles x column tiles (kernel 3: at most one per CU). */
int emd_debug_split32_plan(long M, int Cin, int Cout, unsigned flags, int out[8]);
/* Host only, reads the knobs, touches no device: the plan of the rolling stride-1, rate-1 depthwise launch (csrc/dw_misc.hip,
 * dw3x3_s1_roll / dw3x3_s1_roll_up) -- the function the launchers themselves call.  kind: 0 emd_dw3x3_f32, 1 emd_dw3x3_split32_f32,
 * 2 emd_dw3x3_pre[_act]_f32, 3 emd_dw3x3_pre_split32_f32, 4 emd_dw3x3_reflect_f32, 5 emd_dw3x3_reflect_split32_f32,
 * 6 emd_dw3x3_up_split32_f32.  With wg(t) = B * ceil(H / t) * ceil(W / 16) * ceil(Q / 16) workgroups of t rows, Q = channel quads with a
 * thread (C / 4; ceil32(C) / 4 for a split32 output, whose padding is written too): 16 rows where H >= 64, or H >= 16 and
 * wg(16) >= 1024; else 8, and 4 where wg(8) < 1024; dw_th forces 4, 8, 16 or 32.  REFLECT: 16 where H >= 64, else 8; no knob, launch
 * order.  Returns the strip height, 0 where nothing would be launched (out is then left alone).  out = {strip height, XCD-contiguous
 * tile order (1 / 0), workgroups, strips per image, channel blocks per pixel, Q}. */
int emd_debug_dw_plan(int kind, int B, int H, int W, int C, int out[6]);
/* Device buffer that the split32 GEMM writes s_memtime phase stamps into (NULL = off). */
void emd_debug_split_stamps(void* device_buf);
/* Device buffer that the fused separable conv writes s_memtime phase stamps into (NULL = off). */
void emd_debug_sep_stamps(void* device_buf);
/* The same for emd_sep3x3_gemm_f32 (csrc/sep_gemm.hip): 8 x int64 per workgroup = cycle sums of {own DMA wait, barrier a,
 * depthwise stage, barrier b, fragment reads + DMA issue + MFMAs, -, end stamp, -}. */
void emd_debug_sepgemm_stamps(void* device_buf);


/* On-box peak micro-benchmarks (csrc/dev_bench.hip), timed by bench.py with HIP events (SURVEY.md 8d asks for the measured
 * peaks next to the nominal ones).  emd_stream_t is hipStream_t; return codes as in emdenoise.h. */
/* dst[i] = src[i], n floats (multiple of 4), 16-byte aligned: the read + write stream-copy roof. */
int emd_debug_stream_copy_f32(const float* src, float* dst, long n, void* stream);
/* `workgroups` x 4 waves each issue iters x 32 back-to-back v_mfma_f32_32x32x16_bf16 (32768 flop each) on the 4 KiB of
 * bf16 operands at `ops`; `out` (workgroups x 256 floats) exists to keep the chain alive. */
int emd_debug_mfma_peak_bf16(const void* ops, float* out, int workgroups, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMDENOISE_DEV_H */
