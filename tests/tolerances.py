"""The stated fp32 tolerance of the path (north_star: "within a stated fp32 logit tolerance"), ONE number per stage - DESIGN.md §4 quotes
this file, the GPU parity tests import it (no per-fixture widening of a stage tolerance anywhere else).

Every number bounds  max|hip - ref| / max|ref|  of a stage tensor against the REAL reference's golden values (or the oracle), in every
fp32-grade arithmetic mode (f32, bf16x6, f16x3).

TWO checkpoints, two levels (round 6):

* the WELL-CONDITIONED synthetic checkpoint (vps_amd.synth.conditioned_overrides; golden of the real reference at 1024x2048:
  tests/golden/fusetrack_fullsize_cond.npz): CONDITIONED = 1e-4 for EVERY stage tensor and every detection score - the number
  BASELINE.md section 3 names. Measured: flow 5e-6, FPN 2.5e-6, neck 6e-6 .. 1e-5, semantic logits 7e-6, box-head logits <= 3.7e-5, scores
  1e-6 (profiles/r06_fullsize_conditioned_report.txt). bf16x3 (bf16 operands: what BASELINE config 5 words): 5e-4, measured <= 2.5e-4.

* the plain seeded weights (STAGE below). Behind the FPN that network amplifies rounding noise: fine flows of tens of pixels, deformable
  offsets of several pixels, attention logits of dozens - the fp32 ORACLE itself is 1.9e-4 (1024x2048) from its float64 evaluation at the
  neck (tools/neck_isolation.py, tools/condition_search.py), and the EXACT-fp32 kernels reach 1.7e-3 on one frame of the dense fixture
  (frame 4: neck 1.7e-3, semantic logits 1.9e-3 - in round 5 and in round 6, profiles/r0[56]_fullsize_sep_report.txt). The numbers
  below are what that noise allows, not what the kernels deliver; round 6 tried 1e-3 for the neck and the exact-fp32 mode
  failed it on that frame - the tight gate is the conditioned checkpoint.

  stage                     tolerance   measured (ResNet-50)     note
  flow (FlowNet2, full res)   5e-5      1.5e-6 .. 7.1e-6         5 networks, 60 convolutions: plain summation-order noise
  FPN levels P2..P6           5e-5      1.0e-6 .. 2.9e-6         (same for ResNet-101)
  fusion-neck outputs         2e-3      2.1e-5 .. 1.7e-3
  semantic logits fcn_score   2e-3      6.2e-5 .. 1.9e-3
  cls_score / bbox_pred       2e-3      5.0e-5 .. 9e-4
  detection scores            2e-3      <= 1.54e-3 (absolute: they are probabilities behind a softmax)
  ResNet-101 (config 5): the stages BEHIND the FPN 1e-2: the 101-layer synthetic network amplifies the same noise ~5x, in the exact-fp32
  kernels as much as in the split modes (neck <= 4.5e-3, fcn_score <= 8.2e-3, scores <= 8.3e-3 - all three maxima in bf16x6, the mode
  with the SMALLEST per-product error: summation-order noise, it moves with every change of a split-K partition)

Maps (fraction of differing pixels): semantic 1e-3; panoptic 1e-3, except the two fixtures whose margins cover every LISTING decision but
not which source proposal stands behind a detection - a boundary strip of single instances differs there in every mode, the exact-fp32
kernels included: dense 5e-3 (measured <= 2.6e-3), config5 1.5e-2 (measured <= 6e-3 in round 5, 1.08e-2 in bf16x6 after round 6's uneven
split-K changed the summation order of four decoder layers).

Kernel-level tests of the detection head (tests/test_head_ops_gpu.py) compare exactly, except two bounds that the tests DERIVE from their
own inputs: the distance of a plain float32 restatement of the formula from its float64 evaluation, times a stated factor, never below
the floor. The figures behind them (absolute, measured on the tests' inputs; HEAD_OPS_MEASURED below):

  kernel, case                        float32 restatement vs float64   factor   floor                         bound used
  vps_row_softmax, softmax 5x65           9.7e-8                        4       1e-6 + 1e-5 |ref|             the floor
  vps_row_softmax, softmax 7x129          1.6e-7                        4       1e-6 + 1e-5 |ref|             the floor
  vps_row_softmax, softmax 2x2101         9.6e-8                        4       1e-6 + 1e-5 |ref|             the floor
  vps_row_softmax, log_softmax (all)      3.8e-6                        4       1e-6 + 1e-5 |ref|             max(1.5e-5, floor)
  vps_maskroi_select boxes, n = 37        6.8e-5                        2       1.22e-4 (ulp of width 1024)   1.37e-4
  vps_maskroi_select boxes, n = 1024      9.1e-5                        2       1.22e-4                       1.83e-4
  select -> nms -> finish chain, n = 37   7.9e-5                        2       1.22e-4                       1.58e-4
  (rows of <= 64 columns keep the project's 1e-5 / 1e-6 of tests/test_hip_ops.py)

Kernel-level tests of the panoptic combine and of MaskRemoval (tests/test_pan_ops_gpu.py against tests/pan_restate.py) compare maps and
kept lists exactly. Two bounds decide WHERE: a pixel of a random-input combine case is compared exactly unless the float64 margin
between its two largest logits lies in (0, bound] (then the map must name a channel within bound of the maximum; at most 0.2 % of a
case's pixels may be excluded), and an occupancy pixel of MaskRemoval is compared unless a kept box's resized logit is within
unsure_bound of zero. Both are DERIVED by the tests from their inputs: the factor times the distance of the float32 restatement from
the float64 one, never below the floor (absolute figures, measured on the tests' inputs; PAN_OPS_MEASURED below):

  kernel, case                              float32 restatement vs float64   factor   floor (1 ulp of max |logit|)   bound used   excluded pixels
  combine, k5      (13x22 up 4, k 5)            1.28e-6                        4       9.5e-7                         5.11e-6      0 of 4576
  combine, up2_k70 (20x50 up 2, k 70)           9.07e-7                        4       9.5e-7                         3.63e-6      0 of 4000
  combine, up1_k3  (24x40 up 1, k 3)            3.73e-8                        4       9.5e-7                         the floor    0 of 960
  combine, up8_k12 (5x9 up 8, k 12)             8.79e-7                        4       9.5e-7                         3.52e-6      0 of 2880
  combine, k244    (13x22 up 4, k 244)          1.30e-6                        4       9.5e-7                         5.19e-6      0 of 4576
  combine, c33_k12 (33 classes, k 12)           1.10e-6                        4       9.5e-7                         4.41e-6      0 of 4576
  combine, s7_k12  (S = 7, permuted masks)      1.02e-6                        4       9.5e-7                         4.10e-6      0 of 4576
  MaskRemoval resized logits, n1                9.69e-8                        4       -                              3.87e-7      0 unsure pixels
  MaskRemoval resized logits, n12_c3            6.72e-7                        4       -                              2.69e-6      0
  MaskRemoval resized logits, n40_c2            5.38e-7                        4       -                              2.15e-6      0
  MaskRemoval resized logits, n40_c1            6.39e-7                        4       -                              2.55e-6      0
  MaskRemoval, thr30 / thr31 (all-ones masks)   0                              4       -                              0            0
  (the single-box test of tests/test_hip_ops.py allows 7e-6 max|m28| = about 5e-5 around zero: twenty times these)

Kernel-level tests of the neck and flow glue kernels (tests/test_nn_ops_gpu.py against tests/nn_restate.py, cases in tests/nn_cases.py):
nearest resize, max pool, BFP scatter / scatter_all, the transposes, axpb (one fma) and flow_warp's all-outside zeros compare BITWISE.
Every other case compares with the float64 restatement under bound = max(floor, 4 x max|float32 restatement - float64 restatement|),
floor = one float32 ulp of the case's largest |reference|, DERIVED by the test from its inputs and asserted on the CPU
(tests/test_nn_restate.py) not to exceed the cap = what tests/test_hip_ops.py allows the kernel, atol + rtol max|reference|. Largest figures
per kernel over its bounded cases (absolute; per case in NN_OPS_MEASURED below as (float32 vs float64, bound used, measured max error of the
kernel on an MI355X)):

  kernel          cases  f32 v f64  floor    bound     kernel    cap
  resize            18   4.54e-06 3.81e-06 1.82e-05  4.18e-06  1e-06 + 1e-06 |ref|
  pool              24   3.44e-07 2.38e-07 1.38e-06  3.44e-07  1e-06 + 1e-06 |ref|
  gather             5   1.61e-07 4.77e-07 6.44e-07  1.61e-07  1e-06 + 1e-06 |ref|
  groupnorm         30   2.76e-06 4.77e-07 1.11e-05  5.13e-07  1e-05 + 1e-05 |ref|
  groupnorm          1   12.1     4.77e-07 48.4      3.74e-05  (ill-conditioned by design: relu_C64_G32_p560_relu1_ldv_far_mean)
  groupnorm          1   9.46     4.77e-07 37.8      3.89e-05  (ill-conditioned by design: relu_C2_G1_p560_relu0_ld+4s_far_mean)
  tcea_temporal     12   3.46e-07 2.38e-07 1.38e-06  3.49e-07  1e-05 + 1e-05 |ref|
  tcea_temporal      1   5.95e-06 2.38e-07 2.38e-05  5.95e-06  (ill-conditioned by design: C64_p67_saturated)
  tcea_modulate      3   6.03e-07 4.77e-07 2.41e-06  6.03e-07  1e-06 + 1e-06 |ref|
  resample2d        27   2.83e-07 2.38e-07 1.13e-06  2.38e-07  1e-06 + 1e-06 |ref|
  channelnorm       12   3.85e-07 4.77e-07 1.54e-06  3.85e-07  1e-07 + 1e-06 |ref|
  flow_warp         12   1.36e-05 2.38e-07 5.45e-05  1.36e-05  0.0001 + 0.0001 |ref|
  flow_stage        20   2.12e-06 9.54e-07 8.49e-06  2.11e-06  1e-05 + 1e-05 |ref|
  flow_stage_full    4   3.54e-07 4.77e-07 1.42e-06  2.64e-07  1e-05 + 1e-05 |ref|
  flow_prep         18   6.05e-06 7.63e-06 2.42e-05  3.53e-06  1e-05 + 0 |ref|
  (resize: the large figures belong to alpha = -20, |reference| up to 80; flow_prep: to rgb_mean, values of ~100, cap 1e-4. The two far-mean
  GroupNorm cases are also held to the bound of tests/nn_cases.py groupnorm_affine_bound, 1.9e-2 / 1.4e-2, derived from the number
  formats: measured 3.7e-5 / 3.9e-5; float32 statistics would be off by whole units.)

Kernel-level tests of the correlation kernels (tests/test_corr_gpu.py against tests/corr_restate.py, cases in tests/corr_cases.py: every
kernel instance vps_correlation / vps_correlation_f16 launch at their default switch values, N = 2, channel windows, C up to 1024):
out-of-image displacements compare BITWISE with +0.0, an N = 1 call on image 1 BITWISE with the second half of the N = 2 call, and
vps_correlation_f16 without a matrix-core instance BITWISE with vps_correlation. Everything else compares with the float64 restatement:
the exact kernels under the same derived bound = max(floor, 4 x max|float32 restatement - float64 restatement|), floor = one float32 ulp
of the case's largest |reference|, asserted on the CPU (tests/test_corr_restate.py) not to exceed the cap of tests/test_hip_ops.py,
1e-5 + 1e-5 max|reference|; the split-fp16 matrix-core kernel under the project's figure for it, 2e-6 max|reference|. Largest figures per
kernel over its cases (absolute - the cases' output magnitudes differ by orders, hence the last column; per case in CORR_MEASURED
below as (float32 vs float64, bound used, measured max error of the kernel on an MI355X)):

  kernel                        cases  f32 v f64  floor     bound     kernel    largest kernel / bound of a case
  correlation_kernel<1>            6   3.81e-04  1.95e-03  1.95e-03  1.94e-04  0.48
  correlation_kernel<2>            2   2.54e-05  1.53e-05  1.01e-04  1.82e-05  0.30
  correlation_kernel<4>            3   1.24e-05  7.63e-06  4.95e-05  9.09e-06  0.53
  correlation4_kernel<2,10,1>      6   1.80e-04  6.10e-05  7.21e-04  1.32e-04  0.27
  correlation4h_kernel<4,1>        4   4.76e-06  3.81e-06  1.91e-05  2.96e-06  0.27
  correlation4h_kernel<4,2>        4   5.31e-06  3.81e-06  2.12e-05  6.84e-06  0.34
  correlation_lds_kernel<2,10>     5   2.48e-05  1.53e-05  9.94e-05  6.47e-05  0.79
  corr_mfma_kernel<2,10,8>         4   2.96e-05  1.53e-05  4.81e-04  5.93e-05  0.23   (bound: 2e-6 max|reference|)
  (correlation_lds_kernel sums its channels one after the other in one lane, the restatement pairwise: it comes closest to its bound.
  The first case of correlation_kernel<1> has four channels, one of them scaled by 80: outputs of 2e4.)"""

STAGE = dict(flow=5e-5, fpn=5e-5, neck=2e-3, fcn_score=2e-3, cls_score=2e-3, bbox_pred=2e-3, score=2e-3)
STAGE_R101 = dict(neck=1e-2, fcn_score=1e-2, cls_score=1e-2, bbox_pred=1e-2, score=1e-2)      # the stages behind the FPN of the 101-layer model
# every stage tensor and every detection score on the WELL-CONDITIONED synthetic checkpoint (vps_amd.synth.conditioned_overrides; golden of the
# real reference: tests/golden/fusetrack_fullsize_cond.npz) - the 1e-4 of BASELINE.md section 3
CONDITIONED = 1e-4
# the same for bf16x3 - bf16 operands, 2^-16 per product: the arithmetic BASELINE config 5 names, at the tolerance it can hold (measured <= 2.5e-4)
CONDITIONED_BF16X3 = 5e-4
MAP = dict(sem=1e-3, pan=1e-3, pan_dense=5e-3, pan_config5=1.5e-2)
# what the derived bounds of tests/test_head_ops_gpu.py were derived FROM (a record: the tests recompute them from their inputs)
HEAD_OPS_MEASURED = dict(softmax_f32_vs_f64=1.6e-7, log_softmax_f32_vs_f64=3.8e-6, maskroi_boxes_f32_vs_f64=9.1e-5, maskroi_chain_boxes_f32_vs_f64=7.9e-5)
# the same record for tests/test_pan_ops_gpu.py: the largest float32-vs-float64 distance of the restated logits per case / list
PAN_OPS_MEASURED = dict(combine_f32_vs_f64=dict(k5=1.28e-6, up2_k70=9.07e-7, up1_k3=3.73e-8, up8_k12=8.79e-7, k244=1.30e-6, c33_k12=1.10e-6, s7_k12=1.02e-6),
                        removal_resized_f32_vs_f64=dict(n1=9.69e-8, n12_c3=6.72e-7, n40_c2=5.38e-7, n40_c1=6.39e-7, thr30=0.0, thr31=0.0),
                        combine_excluded_pixels=0, removal_unsure_pixels=0)

# the same record for tests/test_nn_ops_gpu.py, per kernel and case: (max|float32 - float64 restatement|, bound used, max error the kernel showed)
NN_OPS_MEASURED = {
    'resize': {
        'bilinear_7x5_12x9_c8w_a1': (2.41e-07, 9.65e-07, 2.57e-07), 'bilinear_7x5_12x9_c8s_a0.25': (4.56e-08, 1.82e-07, 5.3e-08),
        'bilinear_7x5_12x9_c3_a-20': (3.93e-06, 1.57e-05, 4.18e-06), 'bilinear_33x17_17x9_c8w_a1': (1.92e-07, 7.68e-07, 1.9e-07),
        'bilinear_33x17_17x9_c8s_a0.25': (6.54e-08, 2.62e-07, 5.95e-08), 'bilinear_33x17_17x9_c3_a-20': (3.68e-06, 1.47e-05, 3.58e-06),
        'bilinear_5x9_13x4_c8w_a1': (2.58e-07, 1.03e-06, 1.91e-07), 'bilinear_5x9_13x4_c8s_a0.25': (3.82e-08, 1.53e-07, 3.85e-08),
        'bilinear_5x9_13x4_c3_a-20': (4.54e-06, 1.82e-05, 3.11e-06), 'bilinear_1x6_3x11_c8w_a1': (1.75e-07, 6.99e-07, 8.19e-08),
        'bilinear_1x6_3x11_c8s_a0.25': (3.99e-08, 1.6e-07, 2.61e-08), 'bilinear_1x6_3x11_c3_a-20': (3.33e-06, 1.33e-05, 1.94e-06),
        'bilinear_6x1_4x1_c8w_a1': (5.96e-08, 2.38e-07, 5.96e-08), 'bilinear_6x1_4x1_c8s_a0.25': (2.24e-08, 8.94e-08, 1.86e-08),
        'bilinear_6x1_4x1_c3_a-20': (1.67e-06, 6.68e-06, 1.67e-06), 'bilinear_8x12_8x12_c8w_a1': (0, 2.38e-07, 0),
        'bilinear_8x12_8x12_c8s_a0.25': (0, 5.96e-08, 0), 'bilinear_8x12_8x12_c3_a-20': (1.91e-06, 7.63e-06, 1.91e-06),
    },
    'pool': {
        'avg_1x1_c4w_normal': (3.31e-09, 1.49e-08, 3.31e-09), 'avg_1x1_c4w_negative': (1.32e-08, 5.3e-08, 1.32e-08),
        'avg_1x1_c3_normal': (3.31e-09, 1.49e-08, 3.31e-09), 'avg_1x1_c3_negative': (9.93e-09, 3.97e-08, 9.93e-09),
        'avg_1x7_c4w_normal': (2.98e-08, 1.19e-07, 2.98e-08), 'avg_1x7_c4w_negative': (5.3e-08, 2.12e-07, 5.3e-08),
        'avg_1x7_c3_normal': (2.32e-08, 9.27e-08, 2.32e-08), 'avg_1x7_c3_negative': (5.96e-08, 2.38e-07, 5.96e-08),
        'avg_2x2_c4w_normal': (2.32e-08, 9.27e-08, 2.32e-08), 'avg_2x2_c4w_negative': (4.64e-08, 1.85e-07, 4.64e-08),
        'avg_2x2_c3_normal': (3.31e-08, 1.32e-07, 3.31e-08), 'avg_2x2_c3_negative': (5.3e-08, 2.12e-07, 5.3e-08),
        'avg_2x9_c4w_normal': (2.65e-08, 1.06e-07, 2.65e-08), 'avg_2x9_c4w_negative': (1.06e-07, 4.24e-07, 1.06e-07),
        'avg_2x9_c3_normal': (5.13e-08, 2.05e-07, 5.13e-08), 'avg_2x9_c3_negative': (1.59e-07, 6.36e-07, 1.59e-07),
        'avg_9x2_c4w_normal': (3.64e-08, 1.46e-07, 3.64e-08), 'avg_9x2_c4w_negative': (1.32e-07, 5.3e-07, 1.32e-07),
        'avg_9x2_c3_normal': (3.64e-08, 1.46e-07, 3.64e-08), 'avg_9x2_c3_negative': (1.19e-07, 4.77e-07, 1.19e-07),
        'avg_17x9_c4w_normal': (7.95e-08, 3.18e-07, 7.95e-08), 'avg_17x9_c4w_negative': (3.44e-07, 1.38e-06, 3.44e-07),
        'avg_17x9_c3_normal': (8.32e-08, 3.33e-07, 8.32e-08), 'avg_17x9_c3_negative': (2.78e-07, 1.11e-06, 2.78e-07),
    },
    'gather': {
        'L1': (0, 4.77e-07, 0), 'L2': (1.19e-07, 4.77e-07, 1.19e-07), 'L3': (1.59e-07, 6.36e-07, 1.59e-07), 'L5': (1.61e-07, 6.44e-07, 1.61e-07),
        'r1_3': (1.19e-07, 4.77e-07, 1.19e-07),
    },
    'groupnorm': {
        'relu_C256_G32_p37_relu0_ldv_normal': (6.68e-07, 2.67e-06, 4.26e-07), 'relu_C64_G32_p37_relu1_ldv_normal': (6.46e-07, 2.58e-06, 3.56e-07),
        'relu_C32_G32_p37_relu0_ld+4v_normal': (6.69e-07, 2.68e-06, 3.78e-07), 'relu_C16_G4_p37_relu1_ld+4v_normal': (4.88e-07, 1.95e-06, 2.73e-07),
        'relu_C8_G8_p37_relu0_lds_normal': (4.53e-07, 1.81e-06, 3.08e-07), 'relu_C4_G1_p37_relu1_lds_normal': (2.71e-07, 1.08e-06, 1.52e-07),
        'relu_C4_G4_p37_relu0_ld+4s_normal': (2.61e-07, 1.04e-06, 2.87e-07), 'relu_C2_G1_p37_relu1_ld+4s_normal': (1.57e-07, 6.29e-07, 2.48e-07),
        'relu_C1_G1_p37_relu0_lds_normal': (4.2e-07, 1.68e-06, 2.46e-07), 'relu_C128_G1_p37_relu1_ldv_normal': (4.29e-07, 1.71e-06, 5.13e-07),
        'relu_C64_G32_p1_relu1_ldv_normal': (2.76e-06, 1.11e-05, 2.09e-07), 'relu_C2_G1_p1_relu0_ld+4s_normal': (2.49e-08, 1.19e-07, 2.49e-08),
        'relu_C64_G32_p3_relu0_ld+4s_normal': (6.57e-07, 2.63e-06, 2.52e-07), 'relu_C2_G1_p3_relu1_lds_normal': (1.38e-07, 5.52e-07, 1.88e-08),
        'relu_C64_G32_p560_relu1_ldv_normal': (1.47e-06, 5.86e-06, 4.62e-07), 'relu_C2_G1_p560_relu0_ld+4s_normal': (6.85e-07, 2.74e-06, 2.99e-07),
        'relu_C64_G32_p37_relu1_ld+4v_normal': (6.63e-07, 2.65e-06, 4.07e-07), 'relu_C64_G32_p37_relu0_lds_normal': (4.74e-07, 1.9e-06, 3.25e-07),
        'relu_C2_G1_p37_relu0_lds_normal': (1.29e-07, 5.15e-07, 1.1e-07), 'relu_C64_G32_p37_relu1_ldv_constant': (0, 5.96e-08, 0),
        'relu_C16_G4_p3_relu0_ld+4s_constant': (0, 2.98e-08, 0), 'relu_C2_G1_p37_relu0_lds_constant': (0, 5.96e-08, 0),
        'relu_C64_G32_p560_relu1_ldv_far_mean': (12.1, 48.4, 3.74e-05), 'relu_C2_G1_p560_relu0_ld+4s_far_mean': (9.46, 37.8, 3.89e-05),
        'apply_C16_G4_p37_relu0_ldv_normal_rep1': (4.67e-07, 1.87e-06, 3.95e-07),
        'apply_C16_G4_p37_relu1_ldv_normal_rep1': (4.21e-07, 1.68e-06, 3.06e-07),
        'apply_C16_G4_p37_relu0_lds_normal_rep1': (4.78e-07, 1.91e-06, 2.55e-07),
        'apply_C16_G4_p37_relu1_lds_normal_rep1': (3.02e-07, 1.21e-06, 2.62e-07),
        'apply_C16_G4_p37_relu0_ld+4v_normal_rep3': (4.21e-07, 1.68e-06, 5.02e-07),
        'apply_C16_G4_p37_relu1_ld+4v_normal_rep3': (3.57e-07, 1.43e-06, 3.57e-07),
        'apply_C16_G4_p37_relu0_ld+4s_normal_rep3': (3.37e-07, 1.35e-06, 4.64e-07),
        'apply_C16_G4_p37_relu1_ld+4s_normal_rep3': (3.15e-07, 1.26e-06, 3.13e-07),
    },
    'tcea_temporal': {
        'C4_p1': (4.04e-08, 1.62e-07, 4.04e-08), 'C4_p5': (1.15e-07, 4.6e-07, 8.42e-08), 'C4_p67': (1.29e-07, 5.15e-07, 1.12e-07),
        'C64_p1': (8.73e-08, 3.49e-07, 2.77e-08), 'C64_p5': (2.22e-07, 8.87e-07, 1.06e-07), 'C64_p67': (1.92e-07, 7.66e-07, 1.89e-07),
        'C256_p1': (6.78e-08, 2.71e-07, 9.9e-08), 'C256_p5': (1.83e-07, 7.32e-07, 1.95e-07), 'C256_p67': (2.87e-07, 1.15e-06, 2.87e-07),
        'C512_p1': (2.03e-07, 8.12e-07, 2.03e-07), 'C512_p5': (2.64e-07, 1.06e-06, 2.64e-07), 'C512_p67': (3.46e-07, 1.38e-06, 3.49e-07),
        'C64_p67_saturated': (5.95e-06, 2.38e-05, 5.95e-06),
    },
    'tcea_modulate': {
        'flat_n1': (0, 1.49e-08, 0), 'flat_n1027': (6.03e-07, 2.41e-06, 6.03e-07), 'ld_C8_p37': (4.78e-07, 1.91e-06, 4.78e-07),
    },
    'resample2d': {
        'C1_normal_ccc': (2.83e-07, 1.13e-06, 1.2e-07), 'C1_normal_hhh': (1.35e-07, 5.4e-07, 2.38e-07),
        'C1_normal_hch': (1.44e-07, 5.77e-07, 1.77e-07), 'C1_integer_ccc': (0, 2.38e-07, 0), 'C1_integer_hhh': (0, 2.38e-07, 0),
        'C1_integer_hch': (0, 2.38e-07, 0), 'C1_edges_ccc': (4.47e-08, 2.38e-07, 4.47e-08), 'C1_edges_hhh': (8.94e-08, 3.58e-07, 8.94e-08),
        'C1_edges_hch': (2.98e-08, 1.19e-07, 2.98e-08), 'C3_normal_ccc': (2.1e-07, 8.4e-07, 1.79e-07), 'C3_normal_hhh': (1.86e-07, 7.43e-07, 2.01e-07),
        'C3_normal_hch': (1.97e-07, 7.86e-07, 1.6e-07), 'C3_integer_ccc': (0, 2.38e-07, 0), 'C3_integer_hhh': (0, 2.38e-07, 0),
        'C3_integer_hch': (0, 2.38e-07, 0), 'C3_edges_ccc': (5.96e-08, 2.38e-07, 5.96e-08), 'C3_edges_hhh': (7.82e-08, 3.13e-07, 7.82e-08),
        'C3_edges_hch': (5.96e-08, 2.38e-07, 5.96e-08), 'C5_normal_ccc': (2.65e-07, 1.06e-06, 2.04e-07),
        'C5_normal_hhh': (2.38e-07, 9.54e-07, 2.05e-07), 'C5_normal_hch': (2.38e-07, 9.5e-07, 2.38e-07), 'C5_integer_ccc': (0, 2.38e-07, 0),
        'C5_integer_hhh': (0, 2.38e-07, 0), 'C5_integer_hch': (0, 2.38e-07, 0), 'C5_edges_ccc': (1.19e-07, 4.77e-07, 1.19e-07),
        'C5_edges_hhh': (5.96e-08, 2.38e-07, 5.96e-08), 'C5_edges_hch': (5.96e-08, 2.38e-07, 5.96e-08),
    },
    'channelnorm': {
        'C1_cc': (0, 2.38e-07, 0), 'C1_hh': (0, 2.38e-07, 0), 'C1_hc': (0, 2.38e-07, 0), 'C1_ch': (0, 2.38e-07, 0),
        'C3_cc': (1.73e-07, 6.92e-07, 1.72e-07), 'C3_hh': (1.53e-07, 6.11e-07, 1.53e-07), 'C3_hc': (2.25e-07, 8.99e-07, 1.61e-07),
        'C3_ch': (1.88e-07, 7.51e-07, 1.55e-07), 'C5_cc': (3.85e-07, 1.54e-06, 3.85e-07), 'C5_hh': (2.67e-07, 1.07e-06, 3.77e-07),
        'C5_hc': (2.64e-07, 1.06e-06, 2.64e-07), 'C5_ch': (2.33e-07, 9.33e-07, 2.33e-07),
    },
    'flow_warp': {
        '2x9x7x8_normal': (2.22e-06, 8.87e-06, 1.08e-06), '2x9x7x8_zero': (9.36e-07, 3.75e-06, 1.06e-06),
        '2x9x7x8_edge': (9.47e-07, 3.79e-06, 9.47e-07), '1x24x40x64_normal': (1.36e-05, 5.45e-05, 1.36e-05),
        '1x24x40x64_zero': (1.22e-05, 4.89e-05, 1.22e-05), '1x24x40x64_edge': (9.38e-06, 3.75e-05, 8.07e-06),
        '1x2x2x4_normal': (1.36e-07, 5.45e-07, 1.36e-07), '1x2x2x4_zero': (0, 5.96e-08, 0), '1x2x2x4_edge': (1.58e-07, 6.33e-07, 1.58e-07),
        '2x5x16x12_normal': (2.84e-06, 1.14e-05, 2.6e-06), '2x5x16x12_zero': (2.88e-06, 1.15e-05, 2.91e-06),
        '2x5x16x12_edge': (4.01e-06, 1.6e-05, 4.01e-06),
    },
    'flow_stage': {
        '4x4_up0_div0_all_x6_od0:img': (0, 5.96e-08, 0), '4x4_up0_div0_all_x6_od0:flow': (3.73e-09, 1.19e-07, 0),
        '4x4_up0_div0_all_x6_od0:warp': (1.99e-08, 7.96e-08, 1.96e-08), '4x4_up0_div0_all_x6_od0:diffnorm': (7.62e-08, 3.05e-07, 7.62e-08),
        '4x4_up0_div0_all_x6_od0:flownorm': (4.53e-08, 1.81e-07, 4.53e-08), '4x4_up0_div1_flow_x6_od20:flow': (7.45e-10, 3.73e-09, 7.45e-10),
        '4x4_up1_div0_warp_x8_od0:warp': (1.31e-08, 5.24e-08, 1.24e-08), '4x4_up1_div1_diffnorm_x8_od20:diffnorm': (3.89e-08, 1.56e-07, 5.04e-08),
        '8x12_up0_div0_flownorm_x6_od0:flownorm': (8.33e-07, 3.33e-06, 6.92e-07), '8x12_up0_div1_img_x6_od20:img': (0, 5.96e-08, 0),
        '8x12_up1_div0_all_x8_od0:img': (0, 5.96e-08, 0), '8x12_up1_div0_all_x8_od0:flow': (1.19e-07, 4.77e-07, 1.19e-07),
        '8x12_up1_div0_all_x8_od0:warp': (5.96e-08, 2.38e-07, 5.96e-08), '8x12_up1_div0_all_x8_od0:diffnorm': (8.88e-08, 3.55e-07, 8.88e-08),
        '8x12_up1_div0_all_x8_od0:flownorm': (9.53e-08, 4.77e-07, 1.89e-07), '8x12_up1_div1_flow_x8_od20:flow': (9.54e-09, 3.81e-08, 9.54e-09),
        '20x36_up0_div0_warp_x6_od0:warp': (2.11e-06, 8.44e-06, 2.11e-06), '20x36_up0_div1_diffnorm_x6_od20:diffnorm': (2.12e-06, 8.49e-06, 2.11e-06),
        '20x36_up1_div0_flownorm_x8_od0:flownorm': (8.97e-07, 3.59e-06, 7e-07), '20x36_up1_div1_img_x8_od20:img': (0, 5.96e-08, 0),
    },
    'flow_stage_full': {
        'mode0_4x4': (6.03e-08, 2.41e-07, 6.03e-08), 'mode0_8x12': (3.54e-07, 1.42e-06, 2.64e-07), 'mode1_4x4': (1.45e-07, 5.81e-07, 1.45e-07),
        'mode1_8x12': (1.91e-07, 7.63e-07, 1.91e-07),
    },
    'flow_prep': {
        '5x7_5x7_nblk1_ld8': (6.31e-08, 2.52e-07, 6.9e-08), '5x7_5x7_nblk1_ld8:rgb_mean': (4.46e-06, 1.78e-05, 3.17e-06),
        '5x7_5x7_nblk4_ld12': (7.9e-08, 3.16e-07, 4.87e-08), '5x7_5x7_nblk4_ld12:rgb_mean': (6.05e-06, 2.42e-05, 3.53e-06),
        '5x7_5x7_nblk64_ld8': (6.76e-08, 2.7e-07, 4.21e-08), '5x7_5x7_nblk64_ld8:rgb_mean': (5.14e-06, 2.06e-05, 2.73e-06),
        '5x7_8x16_nblk1_ld12': (7.17e-08, 2.87e-07, 7.47e-08), '5x7_8x16_nblk1_ld12:rgb_mean': (2.03e-06, 8.12e-06, 1.78e-06),
        '5x7_8x16_nblk4_ld8': (7.8e-08, 3.12e-07, 6.6e-08), '5x7_8x16_nblk4_ld8:rgb_mean': (2.05e-06, 8.21e-06, 6.83e-07),
        '5x7_8x16_nblk64_ld12': (5.62e-08, 2.25e-07, 5.62e-08), '5x7_8x16_nblk64_ld12:rgb_mean': (1.29e-06, 5.17e-06, 1.29e-06),
        '16x16_64x64_nblk1_ld8': (1.19e-07, 4.77e-07, 1.19e-07), '16x16_64x64_nblk1_ld8:rgb_mean': (4.83e-07, 1.93e-06, 5.98e-08),
        '16x16_64x64_nblk4_ld12': (9.99e-08, 3.99e-07, 9.99e-08), '16x16_64x64_nblk4_ld12:rgb_mean': (1.91e-07, 9.54e-07, 1.91e-07),
        '16x16_64x64_nblk64_ld8': (1.26e-07, 5.05e-07, 1.01e-07), '16x16_64x64_nblk64_ld8:rgb_mean': (2.79e-07, 1.12e-06, 2.79e-07),
    },
}

# the same record for tests/test_corr_gpu.py, per kernel instance and case: (max|float32 - float64 restatement|, bound used, max error the kernel showed)
CORR_MEASURED = {
    'correlation_kernel<1>': {
        'f32_N2_5x7_C4_md0_s1_ttt': (0.000381, 0.00195, 0.000194), 'f32_N2_5x7_C12_md3_s1_www_leaky': (1.68e-07, 6.72e-07, 3.23e-07),
        'f32_N1_9x11_C64_md4_s1_sst': (4.41e-06, 1.76e-05, 3.75e-06), 'f32_N2_12x20_C256_md20_s2_twt_leaky': (1.26e-05, 5.02e-05, 1.1e-05),
        'f32_N2_7x9_C8_md6_s3_wtw': (5.58e-07, 2.23e-06, 5.58e-07), 'f32_N1_512x516_C4_md1_s1_ttt': (7.3e-06, 2.92e-05, 3.8e-06),
    },
    'correlation_kernel<2>': {
        'f32_N2_4x6_C260_md4_s1_wwt': (2.54e-05, 0.000101, 1.82e-05), 'f32_N1_4x6_C512_md2_s1_ttw_leaky': (5.74e-07, 2.3e-06, 6.95e-07),
    },
    'correlation_kernel<4>': {
        'f32_N2_3x5_C516_md2_s1_ssw': (1.24e-05, 4.95e-05, 9.09e-06), 'f32_N1_3x5_C1024_md4_s1_ttt': (2.68e-06, 1.07e-05, 3.03e-06),
        'f32_N1_3x5_C772_md1_s1_wtt_leaky': (1.12e-06, 4.47e-06, 2.36e-06),
    },
    'correlation4_kernel<2,10,1>': {
        'f32_N2_5x8_C4_md20_s2_ttt': (5.17e-07, 2.07e-06, 4.04e-07), 'f32_N2_7x24_C128_md20_s2_www': (2.2e-06, 8.79e-06, 2.26e-06),
        'f32_N1_3x40_C256_md20_s2_sst_leaky': (2.34e-06, 9.35e-06, 2.54e-06), 'f32_N1_4x16_C36_md20_s2_ttw': (2.04e-06, 8.16e-06, 1.2e-06),
        'f32_N1_2x256_C36_md20_s2_wtt': (3.37e-05, 0.000135, 2.87e-05), 'f16_N1_4x128_C128_md20_s2_ttt': (0.00018, 0.000721, 0.000132),
    },
    'correlation4h_kernel<4,1>': {
        'f32_N2_5x4_C4_md4_s1_ttt': (1.97e-07, 7.87e-07, 1.98e-07), 'f32_N2_9x12_C128_md4_s1_www': (4.76e-06, 1.91e-05, 2.96e-06),
        'f32_N1_6x8_C100_md4_s1_sst_leaky': (1.8e-06, 7.2e-06, 1.11e-06), 'f32_N2_96x172_C8_md4_s1_ttt': (6.44e-07, 2.57e-06, 6.85e-07),
    },
    'correlation4h_kernel<4,2>': {
        'f32_N2_6x8_C132_md4_s1_ttw': (1.77e-06, 7.09e-06, 1.66e-06), 'f32_N1_10x16_C200_md4_s1_www_leaky': (3.76e-06, 1.51e-05, 2e-06),
        'f32_N2_4x12_C256_md4_s1_sst': (5.07e-06, 2.03e-05, 6.84e-06), 'f16_N1_4x64_C256_md4_s1_ttw': (5.31e-06, 2.12e-05, 4.23e-06),
    },
    'correlation_lds_kernel<2,10>': {
        'f32_N2_3x256_C32_md20_s2_ttt': (2.48e-05, 9.94e-05, 6.47e-05), 'f32_N2_3x256_C96_md20_s2_ssw': (2.29e-06, 9.14e-06, 7.24e-06),
        'f32_N1_2x512_C64_md20_s2_wwt_leaky': (3.37e-07, 1.35e-06, 6.93e-07), 'f32_N2_23x256_C32_md20_s2_ttw': (2.62e-06, 1.05e-05, 4.84e-06),
        'f32_N1_1x256_C32_md20_s2_twt': (8.84e-08, 3.53e-07, 1.75e-07),
    },
    'corr_mfma_kernel<2,10,8>': {
        'f16_N2_3x128_C256_md20_s2_ttt': (2.96e-05, 0.000219, 2.7e-05), 'f16_N2_2x256_C256_md20_s2_www': (5.1e-06, 8.62e-05, 2.01e-05),
        'f16_N1_1x128_C256_md20_s2_sst': (1.32e-06, 2.01e-05, 1.7e-06), 'f16_N2_3x128_C256_md20_s2_ttw_leaky': (2.74e-05, 0.000481, 5.93e-05),
    },
}


def stage_tol(name, depth=50):
    """tolerance of a stage tensor by the name the tests report it under (flow, fpn_p2, neck_p6, fcn_score, cls_score, ...)"""
    key = name.split('_p')[0] if name.startswith(('fpn', 'neck')) else name
    return STAGE_R101[key] if depth > 50 and key in STAGE_R101 else STAGE[key]
