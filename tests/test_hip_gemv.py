"""Every decode GEMV kernel (vv_linear with m <= 8) against one fp64 reference, at tiny shapes - through the C ABI only, no engine, no weights.

Each case first asks `vv_linear_route` which kernel its arguments take and asserts the instantiation it means to test.  The cases are generated
(`_cases`) from the launch ladders' rules, restated here as `stream_decide`, `rows_decide` and `lds_decide`: for every instantiation those rules can
reach, under default tuning or under a named `vv_tune` setting, the generator picks the smallest k (units of 512 columns for the streaming kernel,
32- or 64-wide steps for the matrix-core kernel) that selects it, alternating a whole number of units with a ragged end, and walks n, m, the
operands and the layout through the edge forms (n = 1, odd n, n below the block's wave count, broadcast rows, pitches larger than the row ...).
The compiled set is enumerated from the same rules (`ALL_INSTANTIATIONS`, 378 kernels): every one of them is reached by a case, and
`test_built_library_holds_exactly_the_enumerated_kernels` reads the built code objects' symbol tables and finds exactly that set.

The reference (`ref_fp64`) is plain torch fp64 on the operands as the device received them and knows nothing of waves, units or tiles: bf16
weights widened exactly, fp8 codes times row scale, NF4 the effective matrix `quantize_nf4` returns, activations fp32 and unrounded - except on
the matrix-core rows kernel, whose operands are the bf16 pair hi + lo of each activation (vv_gemv_rows.hip): the reference rounds there, once.
Three figures per case: global rel RMS, the worst output row, and the worst element max |out - ref| / rms(ref) - the one that sees a single
wrong column of one row group.

Bars: one constant per route class (BAR), held for all three figures.  `test_bars_sit_between_floor_and_dropped_chunk` (CPU) holds every case to
  bar >= 8 x the case's floor - the error of a torch fp32 stand-in of the same operation (fp32 prologue, fp32 accumulation chunk by 8-column
         chunk) against the fp64 reference; the factor is headroom for another summation order, rsqrtf and expf;
  bar <= 1/10 of what one dropped 8-column K chunk costs an output element's figure (rms over every chunk dropped from every element in turn;
         a single element's single chunk is itself a random sum that can come out near zero).
How each constant was chosen is written at BAR.

Every case lays its operands out with NaN in every pitch gap and two NaN guard rows behind the output, runs twice into separate buffers
(bit-identical; `atomic=1` rows routes are held to the bar only) - ticket split-K routes a third time, which shows the tickets were left
ready - and checks that every in-range output is finite, every gap and guard is still NaN and every input is bit-unchanged.

Measured on the MI355X, largest value over the class's cases (profiles/gemv_parity.txt):
  class     cases      bar     global        row    element  bar / largest
  none        134  3.0e-04   1.80e-07   3.94e-07   1.36e-06          220.9
  rms         199  3.0e-04   2.52e-06   3.40e-06   2.52e-06           88.2
  rms_mod      66  3.0e-04   3.75e-07   1.20e-06   3.75e-06           80.1
  silu         59  3.0e-04   1.59e-06   1.59e-06   2.52e-06          119.0
  rows         11  3.0e-04   1.63e-07   2.68e-07   1.04e-06          288.7
  rows_rms     24  3.0e-04   5.85e-06   6.19e-06   2.59e-05           11.6
None is within a factor of ten of its bar.  The nearest is the rows_rms class's worst element: the matrix-core kernel's bf16 hi + lo pairs come from its
own fp32 prologue, so some differ from the reference's by one step of the low part (2^-17 of the activation).

Instantiation -> case ids (generated: `python tests/test_hip_gemv.py --table`; `test_docstring_table_is_current` keeps it so):
  gemv_stream<m=1,dual=0,ksplit=1,ku=1,rw=1,wq=bf16>   st_bf16_m1_d0_ks1_ku1_rw1_k512_plain   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=1,rw=1,wq=fp8>    st_fp8_m1_d0_ks1_ku1_rw1_k16_rms_b   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=1,rw=2,wq=bf16>   st_bf16_m1_d0_ks1_ku1_rw2_k512_rms_now_res, st_edge_m1_d0_k8_rms_b, ... (4 cases)
  gemv_stream<m=1,dual=0,ksplit=1,ku=1,rw=2,wq=fp8>    st_fp8_m1_d0_ks1_ku1_rw2_k272_rms_mod_gr_inpl
  gemv_stream<m=1,dual=0,ksplit=1,ku=1,rw=4,wq=nf4>    st_nf4_m1_d0_ks1_ku1_rw4_k512_silu_b
  gemv_stream<m=1,dual=0,ksplit=1,ku=2,rw=1,wq=bf16>   st_bf16_m1_d0_ks1_ku2_rw1_k1024_b_gelu_gc_res   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=2,rw=1,wq=fp8>    st_fp8_m1_d0_ks1_ku2_rw1_k528_b_inpl   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=2,rw=2,wq=bf16>   st_bf16_m1_d0_ks1_ku2_rw2_k1024_rms_gelu_gr, st_edge_m1_d0_k520_silu_b
  gemv_stream<m=1,dual=0,ksplit=1,ku=2,rw=2,wq=fp8>    st_fp8_m1_d0_ks1_ku2_rw2_k784_gc_bcast
  gemv_stream<m=1,dual=0,ksplit=1,ku=2,rw=4,wq=nf4>    st_nf4_m1_d0_ks1_ku2_rw4_k1024_rms_b_res_bcast
  gemv_stream<m=1,dual=0,ksplit=1,ku=3,rw=1,wq=bf16>   st_bf16_m1_d0_ks1_ku3_rw1_k1536_plain   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=3,rw=1,wq=fp8>    st_fp8_m1_d0_ks1_ku3_rw1_k1040_rms_b_res_bcast   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=3,rw=2,wq=bf16>   st_bf16_m1_d0_ks1_ku3_rw2_k1536_rms_now_res, st_opt0_m1_d0_k1032_rms_b_gr_res, ... (5 cases)
  gemv_stream<m=1,dual=0,ksplit=1,ku=3,rw=2,wq=fp8>    st_fp8_m1_d0_ks1_ku3_rw2_k1296_rms_mod_gr_inpl
  gemv_stream<m=1,dual=0,ksplit=1,ku=3,rw=4,wq=nf4>    st_nf4_m1_d0_ks1_ku3_rw4_k1536_silu_b
  gemv_stream<m=1,dual=0,ksplit=1,ku=4,rw=1,wq=bf16>   st_bf16_m1_d0_ks1_ku4_rw1_k2048_b_gelu_gc_res   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=4,rw=1,wq=fp8>    st_fp8_m1_d0_ks1_ku4_rw1_k1552_b_inpl   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=4,rw=2,wq=bf16>   st_bf16_m1_d0_ks1_ku4_rw2_k2048_rms_gelu_gr
  gemv_stream<m=1,dual=0,ksplit=1,ku=4,rw=2,wq=fp8>    st_fp8_m1_d0_ks1_ku4_rw2_k1808_gc_bcast
  gemv_stream<m=1,dual=0,ksplit=1,ku=4,rw=4,wq=nf4>    st_nf4_m1_d0_ks1_ku4_rw4_k2048_rms_b_res_bcast
  gemv_stream<m=1,dual=0,ksplit=1,ku=5,rw=1,wq=bf16>   st_bf16_m1_d0_ks1_ku5_rw1_k2560_plain   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=5,rw=1,wq=fp8>    st_fp8_m1_d0_ks1_ku5_rw1_k2064_silu_b   [gemv_small_rw]
  gemv_stream<m=1,dual=0,ksplit=1,ku=5,rw=2,wq=bf16>   st_bf16_m1_d0_ks1_ku5_rw2_k2560_rms_now_res, st_edge_m1_d0_k2560_b_gelu_gc_res
  gemv_stream<m=1,dual=0,ksplit=1,ku=5,rw=2,wq=fp8>    st_fp8_m1_d0_ks1_ku5_rw2_k2320_rms_mod_gr_inpl
  gemv_stream<m=1,dual=0,ksplit=1,ku=5,rw=4,wq=nf4>    st_nf4_m1_d0_ks1_ku5_rw4_k2560_silu_b
  gemv_stream<m=1,dual=0,ksplit=4,ku=2,rw=2,wq=bf16>   st_bf16_m1_d0_ks4_ku2_rw2_k3072_b_gelu_gc_res, st_edge_m1_d0_k2568_b_inpl
  gemv_stream<m=1,dual=0,ksplit=4,ku=2,rw=2,wq=fp8>    st_fp8_m1_d0_ks4_ku2_rw2_k2576_b_inpl
  gemv_stream<m=1,dual=0,ksplit=4,ku=2,rw=4,wq=nf4>    st_nf4_m1_d0_ks4_ku2_rw4_k3072_rms_gelu_gr
  gemv_stream<m=1,dual=0,ksplit=4,ku=3,rw=2,wq=bf16>   st_bf16_m1_d0_ks4_ku3_rw2_k4608_gc_bcast
  gemv_stream<m=1,dual=0,ksplit=4,ku=3,rw=2,wq=fp8>    st_fp8_m1_d0_ks4_ku3_rw2_k4112_rms_b_res_bcast
  gemv_stream<m=1,dual=0,ksplit=4,ku=3,rw=4,wq=nf4>    st_nf4_m1_d0_ks4_ku3_rw4_k4608_plain
  gemv_stream<m=1,dual=0,ksplit=4,ku=4,rw=2,wq=bf16>   st_bf16_m1_d0_ks4_ku4_rw2_k6656_rms_b
  gemv_stream<m=1,dual=0,ksplit=4,ku=4,rw=2,wq=fp8>    st_fp8_m1_d0_ks4_ku4_rw2_k6160_rms_now_res
  gemv_stream<m=1,dual=0,ksplit=4,ku=4,rw=4,wq=nf4>    st_nf4_m1_d0_ks4_ku4_rw4_k6656_rms_mod_gr_inpl
  gemv_stream<m=1,dual=0,ksplit=4,ku=5,rw=2,wq=bf16>   st_bf16_m1_d0_ks4_ku5_rw2_k8704_silu_b, split_m5_k8712_b_gr_res
  gemv_stream<m=1,dual=0,ksplit=4,ku=5,rw=2,wq=fp8>    st_fp8_m1_d0_ks4_ku5_rw2_k8208_b_gelu_gc_res
  gemv_stream<m=1,dual=0,ksplit=4,ku=5,rw=4,wq=nf4>    st_nf4_m1_d0_ks4_ku5_rw4_k8704_b_inpl
  gemv_stream<m=1,dual=0,ksplit=8,ku=2,rw=2,wq=bf16>   st_bf16_m1_d0_ks8_ku2_rw2_k6656_rms_gelu_gr   [gemv_long_ku]
  gemv_stream<m=1,dual=0,ksplit=8,ku=2,rw=2,wq=fp8>    st_fp8_m1_d0_ks8_ku2_rw2_k6160_gc_bcast   [gemv_long_ku]
  gemv_stream<m=1,dual=0,ksplit=8,ku=2,rw=4,wq=nf4>    st_nf4_m1_d0_ks8_ku2_rw4_k6656_rms_b_res_bcast   [gemv_long_ku]
  gemv_stream<m=1,dual=0,ksplit=8,ku=3,rw=2,wq=bf16>   st_bf16_m1_d0_ks8_ku3_rw2_k10752_plain
  gemv_stream<m=1,dual=0,ksplit=8,ku=3,rw=2,wq=fp8>    st_fp8_m1_d0_ks8_ku3_rw2_k10256_rms_b_res_bcast
  gemv_stream<m=1,dual=0,ksplit=8,ku=3,rw=4,wq=nf4>    st_nf4_m1_d0_ks8_ku3_rw4_k10752_rms_now_res
  gemv_stream<m=1,dual=0,ksplit=8,ku=4,rw=2,wq=bf16>   st_bf16_m1_d0_ks8_ku4_rw2_k12800_rms_mod_gr_inpl
  gemv_stream<m=1,dual=0,ksplit=8,ku=4,rw=2,wq=fp8>    st_fp8_m1_d0_ks8_ku4_rw2_k12304_silu_b
  gemv_stream<m=1,dual=0,ksplit=8,ku=4,rw=4,wq=nf4>    st_nf4_m1_d0_ks8_ku4_rw4_k12800_b_gelu_gc_res
  gemv_stream<m=1,dual=0,ksplit=8,ku=5,rw=2,wq=bf16>   st_bf16_m1_d0_ks8_ku5_rw2_k16896_b_inpl
  gemv_stream<m=1,dual=0,ksplit=8,ku=5,rw=2,wq=fp8>    st_fp8_m1_d0_ks8_ku5_rw2_k16400_rms_gelu_gr
  gemv_stream<m=1,dual=0,ksplit=8,ku=5,rw=4,wq=nf4>    st_nf4_m1_d0_ks8_ku5_rw4_k16896_gc_bcast
  gemv_stream<m=1,dual=0,ksplit=16,ku=2,rw=2,wq=bf16>  st_bf16_m1_d0_ks16_ku2_rw2_k12800_rms_b_res_bcast, st_ks16_waves_13_to_15_no_unit   [gemv_long_ku]
  gemv_stream<m=1,dual=0,ksplit=16,ku=2,rw=2,wq=fp8>   st_fp8_m1_d0_ks16_ku2_rw2_k12304_plain   [gemv_long_ku]
  gemv_stream<m=1,dual=0,ksplit=16,ku=3,rw=2,wq=bf16>  st_bf16_m1_d0_ks16_ku3_rw2_k20992_silu_b
  gemv_stream<m=1,dual=0,ksplit=16,ku=3,rw=2,wq=fp8>   st_fp8_m1_d0_ks16_ku3_rw2_k20496_rms_now_res
  gemv_stream<m=1,dual=0,ksplit=16,ku=4,rw=2,wq=bf16>  st_bf16_m1_d0_ks16_ku4_rw2_k25088_rms_mod_gr_inpl
  gemv_stream<m=1,dual=0,ksplit=16,ku=4,rw=2,wq=fp8>   st_fp8_m1_d0_ks16_ku4_rw2_k24592_silu_b
  gemv_stream<m=1,dual=0,ksplit=16,ku=5,rw=2,wq=bf16>  st_bf16_m1_d0_ks16_ku5_rw2_k33280_b_gelu_gc_res
  gemv_stream<m=1,dual=0,ksplit=16,ku=5,rw=2,wq=fp8>   st_fp8_m1_d0_ks16_ku5_rw2_k32784_b_inpl
  gemv_stream<m=1,dual=1,ksplit=1,ku=1,rw=1,wq=bf16>   st_bf16_m1_d1_ks1_ku1_rw1_k504_rms_now_swiglu_inpl
  gemv_stream<m=1,dual=1,ksplit=1,ku=1,rw=1,wq=fp8>    st_fp8_m1_d1_ks1_ku1_rw1_k512_silu_b_swiglu
  gemv_stream<m=1,dual=1,ksplit=1,ku=1,rw=2,wq=bf16>   st_bf16_m1_d1_ks1_ku1_rw2_k8_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=1,rw=2,wq=fp8>    st_fp8_m1_d1_ks1_ku1_rw2_k512_rms_swiglu   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=1,rw=4,wq=nf4>    st_nf4_m1_d1_ks1_ku1_rw4_k256_rms_now_swiglu_inpl
  gemv_stream<m=1,dual=1,ksplit=1,ku=2,rw=1,wq=bf16>   st_bf16_m1_d1_ks1_ku2_rw1_k1016_rms_mod_swiglu_gc, split_m5_dual_k520_swiglu_gr_inpl
  gemv_stream<m=1,dual=1,ksplit=1,ku=2,rw=1,wq=fp8>    st_fp8_m1_d1_ks1_ku2_rw1_k1024_rms_now_swiglu_inpl
  gemv_stream<m=1,dual=1,ksplit=1,ku=2,rw=2,wq=bf16>   st_bf16_m1_d1_ks1_ku2_rw2_k520_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=2,rw=2,wq=fp8>    st_fp8_m1_d1_ks1_ku2_rw2_k1024_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=2,rw=4,wq=nf4>    st_nf4_m1_d1_ks1_ku2_rw4_k768_rms_swiglu
  gemv_stream<m=1,dual=1,ksplit=1,ku=3,rw=1,wq=bf16>   st_bf16_m1_d1_ks1_ku3_rw1_k1528_swiglu_gr_res
  gemv_stream<m=1,dual=1,ksplit=1,ku=3,rw=1,wq=fp8>    st_fp8_m1_d1_ks1_ku3_rw1_k1536_rms_mod_swiglu_gc
  gemv_stream<m=1,dual=1,ksplit=1,ku=3,rw=2,wq=bf16>   st_bf16_m1_d1_ks1_ku3_rw2_k1032_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=3,rw=2,wq=fp8>    st_fp8_m1_d1_ks1_ku3_rw2_k1536_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=3,rw=4,wq=nf4>    st_nf4_m1_d1_ks1_ku3_rw4_k1280_rms_swiglu_bcast
  gemv_stream<m=1,dual=1,ksplit=1,ku=4,rw=1,wq=bf16>   st_bf16_m1_d1_ks1_ku4_rw1_k2040_rms_swiglu
  gemv_stream<m=1,dual=1,ksplit=1,ku=4,rw=1,wq=fp8>    st_fp8_m1_d1_ks1_ku4_rw1_k2048_swiglu_gr_res
  gemv_stream<m=1,dual=1,ksplit=1,ku=4,rw=2,wq=bf16>   st_bf16_m1_d1_ks1_ku4_rw2_k1544_rms_mod_swiglu_gc   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=4,rw=2,wq=fp8>    st_fp8_m1_d1_ks1_ku4_rw2_k2048_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=4,rw=4,wq=nf4>    st_nf4_m1_d1_ks1_ku4_rw4_k1792_silu_b_swiglu
  gemv_stream<m=1,dual=1,ksplit=1,ku=5,rw=1,wq=bf16>   st_bf16_m1_d1_ks1_ku5_rw1_k2552_rms_swiglu_bcast
  gemv_stream<m=1,dual=1,ksplit=1,ku=5,rw=1,wq=fp8>    st_fp8_m1_d1_ks1_ku5_rw1_k2560_rms_swiglu
  gemv_stream<m=1,dual=1,ksplit=1,ku=5,rw=2,wq=bf16>   st_bf16_m1_d1_ks1_ku5_rw2_k2056_swiglu_gr_res   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=1,ku=5,rw=2,wq=fp8>    st_fp8_m1_d1_ks1_ku5_rw2_k2560_rms_mod_swiglu_gc   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=4,ku=2,rw=1,wq=bf16>   st_bf16_m1_d1_ks4_ku2_rw1_k2824_rms_now_swiglu_inpl
  gemv_stream<m=1,dual=1,ksplit=4,ku=2,rw=1,wq=fp8>    st_fp8_m1_d1_ks4_ku2_rw1_k3072_silu_b_swiglu
  gemv_stream<m=1,dual=1,ksplit=4,ku=2,rw=2,wq=bf16>   st_bf16_m1_d1_ks4_ku2_rw2_k3064_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=4,ku=2,rw=2,wq=fp8>    st_fp8_m1_d1_ks4_ku2_rw2_k3072_rms_swiglu   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=4,ku=2,rw=4,wq=nf4>    st_nf4_m1_d1_ks4_ku2_rw4_k2112_swiglu_gr_res
  gemv_stream<m=1,dual=1,ksplit=4,ku=3,rw=1,wq=bf16>   st_bf16_m1_d1_ks4_ku3_rw1_k4360_rms_mod_swiglu_gc
  gemv_stream<m=1,dual=1,ksplit=4,ku=3,rw=1,wq=fp8>    st_fp8_m1_d1_ks4_ku3_rw1_k4608_rms_now_swiglu_inpl
  gemv_stream<m=1,dual=1,ksplit=4,ku=3,rw=2,wq=bf16>   st_bf16_m1_d1_ks4_ku3_rw2_k4600_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=4,ku=3,rw=2,wq=fp8>    st_fp8_m1_d1_ks4_ku3_rw2_k4608_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=4,ku=3,rw=4,wq=nf4>    st_nf4_m1_d1_ks4_ku3_rw4_k4160_rms_swiglu
  gemv_stream<m=1,dual=1,ksplit=8,ku=2,rw=1,wq=bf16>   st_bf16_m1_d1_ks8_ku2_rw1_k6408_rms_swiglu_bcast
  gemv_stream<m=1,dual=1,ksplit=8,ku=2,rw=1,wq=fp8>    st_fp8_m1_d1_ks8_ku2_rw1_k6656_rms_mod_swiglu_gc
  gemv_stream<m=1,dual=1,ksplit=8,ku=2,rw=2,wq=bf16>   st_bf16_m1_d1_ks8_ku2_rw2_k6648_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=8,ku=2,rw=2,wq=fp8>    st_fp8_m1_d1_ks8_ku2_rw2_k6656_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=8,ku=2,rw=4,wq=nf4>    st_nf4_m1_d1_ks8_ku2_rw4_k6208_rms_swiglu_bcast
  gemv_stream<m=1,dual=1,ksplit=8,ku=3,rw=1,wq=bf16>   st_bf16_m1_d1_ks8_ku3_rw1_k8456_rms_swiglu
  gemv_stream<m=1,dual=1,ksplit=8,ku=3,rw=1,wq=fp8>    st_fp8_m1_d1_ks8_ku3_rw1_k8704_swiglu_gr_res
  gemv_stream<m=1,dual=1,ksplit=8,ku=3,rw=2,wq=bf16>   st_bf16_m1_d1_ks8_ku3_rw2_k8696_rms_mod_swiglu_gc   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=8,ku=3,rw=2,wq=fp8>    st_fp8_m1_d1_ks8_ku3_rw2_k8704_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=1,dual=1,ksplit=8,ku=3,rw=4,wq=nf4>    st_nf4_m1_d1_ks8_ku3_rw4_k8256_silu_b_swiglu
  gemv_stream<m=2,dual=0,ksplit=1,ku=1,rw=1,wq=bf16>   st_bf16_m2_d0_ks1_ku1_rw1_k512_rms_b   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=1,rw=1,wq=fp8>    st_fp8_m2_d0_ks1_ku1_rw1_k496_rms_now_res   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=1,rw=2,wq=bf16>   st_bf16_m2_d0_ks1_ku1_rw2_k512_rms_mod_gr_inpl
  gemv_stream<m=2,dual=0,ksplit=1,ku=1,rw=2,wq=fp8>    st_fp8_m2_d0_ks1_ku1_rw2_k16_silu_b
  gemv_stream<m=2,dual=0,ksplit=1,ku=1,rw=4,wq=nf4>    st_nf4_m2_d0_ks1_ku1_rw4_k512_b_gelu_gc_res
  gemv_stream<m=2,dual=0,ksplit=1,ku=2,rw=1,wq=bf16>   st_bf16_m2_d0_ks1_ku2_rw1_k1024_b_inpl   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=2,rw=1,wq=fp8>    st_fp8_m2_d0_ks1_ku2_rw1_k1008_rms_gelu_gr   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=2,rw=2,wq=bf16>   st_bf16_m2_d0_ks1_ku2_rw2_k1024_gc_bcast, st_pers3_bf16_d0_k1024_silu_b
  gemv_stream<m=2,dual=0,ksplit=1,ku=2,rw=2,wq=fp8>    st_fp8_m2_d0_ks1_ku2_rw2_k528_rms_b_res_bcast, st_pers3_fp8_d0_k1024_silu_b
  gemv_stream<m=2,dual=0,ksplit=1,ku=2,rw=4,wq=nf4>    st_nf4_m2_d0_ks1_ku2_rw4_k1024_plain, st_pers3_nf4_d0_k1024_silu_b
  gemv_stream<m=2,dual=0,ksplit=1,ku=3,rw=1,wq=bf16>   st_bf16_m2_d0_ks1_ku3_rw1_k1536_rms_b   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=3,rw=1,wq=fp8>    st_fp8_m2_d0_ks1_ku3_rw1_k1520_rms_now_res   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=3,rw=2,wq=bf16>   st_bf16_m2_d0_ks1_ku3_rw2_k1536_rms_mod_gr_inpl
  gemv_stream<m=2,dual=0,ksplit=1,ku=3,rw=2,wq=fp8>    st_fp8_m2_d0_ks1_ku3_rw2_k1040_silu_b
  gemv_stream<m=2,dual=0,ksplit=1,ku=3,rw=4,wq=nf4>    st_nf4_m2_d0_ks1_ku3_rw4_k1536_b_gelu_gc_res
  gemv_stream<m=2,dual=0,ksplit=1,ku=4,rw=1,wq=bf16>   st_bf16_m2_d0_ks1_ku4_rw1_k2048_b_inpl   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=4,rw=1,wq=fp8>    st_fp8_m2_d0_ks1_ku4_rw1_k2032_rms_gelu_gr   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=4,rw=2,wq=bf16>   st_bf16_m2_d0_ks1_ku4_rw2_k2048_gc_bcast, st_waves3_m2_d0_n10, ... (5 cases)
  gemv_stream<m=2,dual=0,ksplit=1,ku=4,rw=2,wq=fp8>    st_fp8_m2_d0_ks1_ku4_rw2_k1552_rms_b_res_bcast
  gemv_stream<m=2,dual=0,ksplit=1,ku=4,rw=4,wq=nf4>    st_nf4_m2_d0_ks1_ku4_rw4_k2048_plain
  gemv_stream<m=2,dual=0,ksplit=1,ku=5,rw=1,wq=bf16>   st_bf16_m2_d0_ks1_ku5_rw1_k2312_rms_b   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=5,rw=1,wq=fp8>    st_fp8_m2_d0_ks1_ku5_rw1_k2560_rms_now_res   [gemv_small_rw]
  gemv_stream<m=2,dual=0,ksplit=1,ku=5,rw=2,wq=bf16>   st_bf16_m2_d0_ks1_ku5_rw2_k2552_rms_mod_gr_inpl
  gemv_stream<m=2,dual=0,ksplit=1,ku=5,rw=2,wq=fp8>    st_fp8_m2_d0_ks1_ku5_rw2_k2560_silu_b
  gemv_stream<m=2,dual=0,ksplit=1,ku=5,rw=4,wq=nf4>    st_nf4_m2_d0_ks1_ku5_rw4_k2112_b_gelu_gc_res
  gemv_stream<m=2,dual=0,ksplit=4,ku=2,rw=2,wq=bf16>   st_bf16_m2_d0_ks4_ku2_rw2_k3072_b_inpl, st_pers3_bf16_d0_k3520_plain
  gemv_stream<m=2,dual=0,ksplit=4,ku=2,rw=2,wq=fp8>    st_fp8_m2_d0_ks4_ku2_rw2_k2832_rms_gelu_gr, st_pers3_fp8_d0_k3520_plain
  gemv_stream<m=2,dual=0,ksplit=4,ku=2,rw=4,wq=nf4>    st_nf4_m2_d0_ks4_ku2_rw4_k3072_gc_bcast, st_pers3_nf4_d0_k3520_plain
  gemv_stream<m=2,dual=0,ksplit=4,ku=3,rw=2,wq=bf16>   st_bf16_m2_d0_ks4_ku3_rw2_k4608_rms_b_res_bcast, st_ks4_ku3_wave1_idle_k4608_gc_bcast
  gemv_stream<m=2,dual=0,ksplit=4,ku=3,rw=2,wq=fp8>    st_fp8_m2_d0_ks4_ku3_rw2_k4368_plain
  gemv_stream<m=2,dual=0,ksplit=4,ku=3,rw=4,wq=nf4>    st_nf4_m2_d0_ks4_ku3_rw4_k4608_rms_b
  gemv_stream<m=2,dual=0,ksplit=4,ku=4,rw=2,wq=bf16>   st_bf16_m2_d0_ks4_ku4_rw2_k6408_rms_now_res, st_lastpartial_k6152_rms_now_res
  gemv_stream<m=2,dual=0,ksplit=4,ku=4,rw=2,wq=fp8>    st_fp8_m2_d0_ks4_ku4_rw2_k6656_rms_mod_gr_inpl
  gemv_stream<m=2,dual=0,ksplit=4,ku=4,rw=4,wq=nf4>    st_nf4_m2_d0_ks4_ku4_rw4_k6592_silu_b
  gemv_stream<m=2,dual=0,ksplit=4,ku=5,rw=2,wq=bf16>   st_bf16_m2_d0_ks4_ku5_rw2_k8456_b_gelu_gc_res, st_ks8_ku3_7idle_k8704_silu_b, ... (3 cases)
  gemv_stream<m=2,dual=0,ksplit=4,ku=5,rw=2,wq=fp8>    st_fp8_m2_d0_ks4_ku5_rw2_k8704_b_inpl
  gemv_stream<m=2,dual=0,ksplit=4,ku=5,rw=4,wq=nf4>    st_nf4_m2_d0_ks4_ku5_rw4_k8640_rms_gelu_gr
  gemv_stream<m=2,dual=0,ksplit=8,ku=2,rw=2,wq=bf16>   st_bf16_m2_d0_ks8_ku2_rw2_k6656_gc_bcast   [gemv_long_ku]
  gemv_stream<m=2,dual=0,ksplit=8,ku=2,rw=2,wq=fp8>    st_fp8_m2_d0_ks8_ku2_rw2_k6416_rms_b_res_bcast   [gemv_long_ku]
  gemv_stream<m=2,dual=0,ksplit=8,ku=2,rw=4,wq=nf4>    st_nf4_m2_d0_ks8_ku2_rw4_k6656_plain   [gemv_long_ku]
  gemv_stream<m=2,dual=0,ksplit=8,ku=3,rw=2,wq=bf16>   st_bf16_m2_d0_ks8_ku3_rw2_k10752_rms_b, st_ks8_lastpartial_k10504_silu_b
  gemv_stream<m=2,dual=0,ksplit=8,ku=3,rw=2,wq=fp8>    st_fp8_m2_d0_ks8_ku3_rw2_k10512_rms_now_res
  gemv_stream<m=2,dual=0,ksplit=8,ku=3,rw=4,wq=nf4>    st_nf4_m2_d0_ks8_ku3_rw4_k10752_rms_mod_gr_inpl
  gemv_stream<m=2,dual=0,ksplit=8,ku=4,rw=2,wq=bf16>   st_bf16_m2_d0_ks8_ku4_rw2_k12552_silu_b
  gemv_stream<m=2,dual=0,ksplit=8,ku=4,rw=2,wq=fp8>    st_fp8_m2_d0_ks8_ku4_rw2_k12800_b_gelu_gc_res
  gemv_stream<m=2,dual=0,ksplit=8,ku=4,rw=4,wq=nf4>    st_nf4_m2_d0_ks8_ku4_rw4_k12736_b_inpl
  gemv_stream<m=2,dual=0,ksplit=8,ku=5,rw=2,wq=bf16>   st_bf16_m2_d0_ks8_ku5_rw2_k16648_rms_gelu_gr
  gemv_stream<m=2,dual=0,ksplit=8,ku=5,rw=2,wq=fp8>    st_fp8_m2_d0_ks8_ku5_rw2_k16896_gc_bcast
  gemv_stream<m=2,dual=0,ksplit=8,ku=5,rw=4,wq=nf4>    st_nf4_m2_d0_ks8_ku5_rw4_k16832_rms_b_res_bcast
  gemv_stream<m=2,dual=0,ksplit=16,ku=2,rw=2,wq=bf16>  st_bf16_m2_d0_ks16_ku2_rw2_k12800_plain   [gemv_long_ku]
  gemv_stream<m=2,dual=0,ksplit=16,ku=2,rw=2,wq=fp8>   st_fp8_m2_d0_ks16_ku2_rw2_k12560_rms_b   [gemv_long_ku]
  gemv_stream<m=2,dual=0,ksplit=16,ku=3,rw=2,wq=bf16>  st_bf16_m2_d0_ks16_ku3_rw2_k20992_rms_now_res, st_ks16_lastpartial_k21256_b_inpl
  gemv_stream<m=2,dual=0,ksplit=16,ku=3,rw=2,wq=fp8>   st_fp8_m2_d0_ks16_ku3_rw2_k20752_rms_mod_gr_inpl
  gemv_stream<m=2,dual=0,ksplit=16,ku=4,rw=2,wq=bf16>  st_bf16_m2_d0_ks16_ku4_rw2_k25088_silu_b
  gemv_stream<m=2,dual=0,ksplit=16,ku=4,rw=2,wq=fp8>   st_fp8_m2_d0_ks16_ku4_rw2_k24848_b_gelu_gc_res
  gemv_stream<m=2,dual=0,ksplit=16,ku=5,rw=2,wq=bf16>  st_bf16_m2_d0_ks16_ku5_rw2_k33280_b_inpl
  gemv_stream<m=2,dual=0,ksplit=16,ku=5,rw=2,wq=fp8>   st_fp8_m2_d0_ks16_ku5_rw2_k33040_rms_gelu_gr
  gemv_stream<m=2,dual=1,ksplit=1,ku=1,rw=1,wq=bf16>   st_bf16_m2_d1_ks1_ku1_rw1_k264_rms_mod_swiglu_gc, st_edge_m2_d1_k8_rms_mod_swiglu_gc, ... (4 cases)
  gemv_stream<m=2,dual=1,ksplit=1,ku=1,rw=1,wq=fp8>    st_fp8_m2_d1_ks1_ku1_rw1_k512_rms_now_swiglu_inpl
  gemv_stream<m=2,dual=1,ksplit=1,ku=1,rw=2,wq=bf16>   st_bf16_m2_d1_ks1_ku1_rw2_k504_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=1,rw=2,wq=fp8>    st_fp8_m2_d1_ks1_ku1_rw2_k512_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=1,rw=4,wq=nf4>    st_nf4_m2_d1_ks1_ku1_rw4_k64_rms_swiglu
  gemv_stream<m=2,dual=1,ksplit=1,ku=2,rw=1,wq=bf16>   st_bf16_m2_d1_ks1_ku2_rw1_k776_swiglu_gr_res, st_edge_m2_d1_k520_rms_swiglu_bcast, ... (4 cases)
  gemv_stream<m=2,dual=1,ksplit=1,ku=2,rw=1,wq=fp8>    st_fp8_m2_d1_ks1_ku2_rw1_k1024_rms_mod_swiglu_gc, st_pers3_fp8_d1_k1024_rms_swiglu_bcast
  gemv_stream<m=2,dual=1,ksplit=1,ku=2,rw=2,wq=bf16>   st_bf16_m2_d1_ks1_ku2_rw2_k1016_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=2,rw=2,wq=fp8>    st_fp8_m2_d1_ks1_ku2_rw2_k1024_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=2,rw=4,wq=nf4>    st_nf4_m2_d1_ks1_ku2_rw4_k576_rms_swiglu_bcast, st_pers3_nf4_d1_k1024_rms_swiglu_bcast
  gemv_stream<m=2,dual=1,ksplit=1,ku=3,rw=1,wq=bf16>   st_bf16_m2_d1_ks1_ku3_rw1_k1288_rms_swiglu, st_opt0_m2_d1_k1032_rms_b_swiglu_gr_res, ... (5 cases)
  gemv_stream<m=2,dual=1,ksplit=1,ku=3,rw=1,wq=fp8>    st_fp8_m2_d1_ks1_ku3_rw1_k1536_swiglu_gr_res
  gemv_stream<m=2,dual=1,ksplit=1,ku=3,rw=2,wq=bf16>   st_bf16_m2_d1_ks1_ku3_rw2_k1528_rms_mod_swiglu_gc   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=3,rw=2,wq=fp8>    st_fp8_m2_d1_ks1_ku3_rw2_k1536_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=3,rw=4,wq=nf4>    st_nf4_m2_d1_ks1_ku3_rw4_k1088_silu_b_swiglu
  gemv_stream<m=2,dual=1,ksplit=1,ku=4,rw=1,wq=bf16>   st_bf16_m2_d1_ks1_ku4_rw1_k1800_rms_swiglu_bcast, st_waves3_m2_d1_n10, ... (5 cases)
  gemv_stream<m=2,dual=1,ksplit=1,ku=4,rw=1,wq=fp8>    st_fp8_m2_d1_ks1_ku4_rw1_k2048_rms_swiglu
  gemv_stream<m=2,dual=1,ksplit=1,ku=4,rw=2,wq=bf16>   st_bf16_m2_d1_ks1_ku4_rw2_k2040_swiglu_gr_res   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=4,rw=2,wq=fp8>    st_fp8_m2_d1_ks1_ku4_rw2_k2048_rms_mod_swiglu_gc   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=4,rw=4,wq=nf4>    st_nf4_m2_d1_ks1_ku4_rw4_k1600_rms_now_swiglu_inpl
  gemv_stream<m=2,dual=1,ksplit=1,ku=5,rw=1,wq=bf16>   st_bf16_m2_d1_ks1_ku5_rw1_k2560_silu_b_swiglu, st_edge_m2_d1_k2560_rms_swiglu
  gemv_stream<m=2,dual=1,ksplit=1,ku=5,rw=1,wq=fp8>    st_fp8_m2_d1_ks1_ku5_rw1_k2320_rms_swiglu_bcast
  gemv_stream<m=2,dual=1,ksplit=1,ku=5,rw=2,wq=bf16>   st_bf16_m2_d1_ks1_ku5_rw2_k2560_rms_swiglu   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=1,ku=5,rw=2,wq=fp8>    st_fp8_m2_d1_ks1_ku5_rw2_k2544_swiglu_gr_res   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=4,ku=2,rw=1,wq=bf16>   st_bf16_m2_d1_ks4_ku2_rw1_k3064_rms_mod_swiglu_gc, st_edge_m2_d1_k2568_swiglu_gr_res, ... (7 cases)
  gemv_stream<m=2,dual=1,ksplit=4,ku=2,rw=1,wq=fp8>    st_fp8_m2_d1_ks4_ku2_rw1_k3072_rms_now_swiglu_inpl, st_pers3_fp8_d1_k3520_rms_swiglu_bcast
  gemv_stream<m=2,dual=1,ksplit=4,ku=2,rw=2,wq=bf16>   st_bf16_m2_d1_ks4_ku2_rw2_k2568_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=4,ku=2,rw=2,wq=fp8>    st_fp8_m2_d1_ks4_ku2_rw2_k3072_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=4,ku=2,rw=4,wq=nf4>    st_nf4_m2_d1_ks4_ku2_rw4_k2304_rms_swiglu, st_nf4_dual_5units, ... (3 cases)
  gemv_stream<m=2,dual=1,ksplit=4,ku=3,rw=1,wq=bf16>   st_bf16_m2_d1_ks4_ku3_rw1_k4600_swiglu_gr_res
  gemv_stream<m=2,dual=1,ksplit=4,ku=3,rw=1,wq=fp8>    st_fp8_m2_d1_ks4_ku3_rw1_k4608_rms_mod_swiglu_gc
  gemv_stream<m=2,dual=1,ksplit=4,ku=3,rw=2,wq=bf16>   st_bf16_m2_d1_ks4_ku3_rw2_k4104_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=4,ku=3,rw=2,wq=fp8>    st_fp8_m2_d1_ks4_ku3_rw2_k4608_silu_b_swiglu   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=4,ku=3,rw=4,wq=nf4>    st_nf4_m2_d1_ks4_ku3_rw4_k4352_rms_swiglu_bcast
  gemv_stream<m=2,dual=1,ksplit=8,ku=2,rw=1,wq=bf16>   st_bf16_m2_d1_ks8_ku2_rw1_k6648_rms_swiglu
  gemv_stream<m=2,dual=1,ksplit=8,ku=2,rw=1,wq=fp8>    st_fp8_m2_d1_ks8_ku2_rw1_k6656_swiglu_gr_res
  gemv_stream<m=2,dual=1,ksplit=8,ku=2,rw=2,wq=bf16>   st_bf16_m2_d1_ks8_ku2_rw2_k6152_rms_mod_swiglu_gc   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=8,ku=2,rw=2,wq=fp8>    st_fp8_m2_d1_ks8_ku2_rw2_k6656_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=8,ku=2,rw=4,wq=nf4>    st_nf4_m2_d1_ks8_ku2_rw4_k6400_silu_b_swiglu
  gemv_stream<m=2,dual=1,ksplit=8,ku=3,rw=1,wq=bf16>   st_bf16_m2_d1_ks8_ku3_rw1_k8696_rms_swiglu_bcast
  gemv_stream<m=2,dual=1,ksplit=8,ku=3,rw=1,wq=fp8>    st_fp8_m2_d1_ks8_ku3_rw1_k8704_rms_swiglu
  gemv_stream<m=2,dual=1,ksplit=8,ku=3,rw=2,wq=bf16>   st_bf16_m2_d1_ks8_ku3_rw2_k8200_swiglu_gr_res   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=8,ku=3,rw=2,wq=fp8>    st_fp8_m2_d1_ks8_ku3_rw2_k8704_rms_mod_swiglu_gc   [gemv_dual_rw]
  gemv_stream<m=2,dual=1,ksplit=8,ku=3,rw=4,wq=nf4>    st_nf4_m2_d1_ks8_ku3_rw4_k8448_rms_now_swiglu_inpl
  gemv_stream<m=4,dual=0,ksplit=1,ku=1,rw=1,wq=bf16>   st_bf16_m4_d0_ks1_ku1_rw1_k512_rms_now_res   [gemv_small_rw]
  gemv_stream<m=4,dual=0,ksplit=1,ku=1,rw=2,wq=bf16>   st_bf16_m3_d0_ks1_ku1_rw2_k264_rms_mod_gr_inpl, st_edge_m3_d0_k8_rms_mod_gr_inpl, ... (4 cases)
  gemv_stream<m=4,dual=0,ksplit=1,ku=2,rw=1,wq=bf16>   st_bf16_m4_d0_ks1_ku2_rw1_k1024_silu_b   [gemv_small_rw]
  gemv_stream<m=4,dual=0,ksplit=1,ku=2,rw=2,wq=bf16>   st_bf16_m3_d0_ks1_ku2_rw2_k776_b_gelu_gc_res, st_edge_m3_d0_k520_b_inpl
  gemv_stream<m=4,dual=0,ksplit=1,ku=3,rw=1,wq=bf16>   st_bf16_m4_d0_ks1_ku3_rw1_k1536_b_inpl   [gemv_small_rw]
  gemv_stream<m=4,dual=0,ksplit=1,ku=3,rw=2,wq=bf16>   st_bf16_m3_d0_ks1_ku3_rw2_k1288_rms_gelu_gr
  gemv_stream<m=4,dual=0,ksplit=1,ku=4,rw=1,wq=bf16>   st_bf16_m4_d0_ks1_ku4_rw1_k2048_gc_bcast   [gemv_small_rw]
  gemv_stream<m=4,dual=0,ksplit=1,ku=4,rw=2,wq=bf16>   st_bf16_m3_d0_ks1_ku4_rw2_k1800_rms_b_res_bcast
  gemv_stream<m=4,dual=0,ksplit=1,ku=5,rw=1,wq=bf16>   st_bf16_m4_d0_ks1_ku5_rw1_k2560_plain   [gemv_small_rw]
  gemv_stream<m=4,dual=0,ksplit=1,ku=5,rw=2,wq=bf16>   st_bf16_m3_d0_ks1_ku5_rw2_k2056_rms_b, st_edge_m3_d0_k2560_rms_gelu_gr
  gemv_stream<m=4,dual=0,ksplit=4,ku=2,rw=2,wq=bf16>   st_bf16_m4_d0_ks4_ku2_rw2_k3072_rms_now_res, st_edge_m3_d0_k2568_gc_bcast, ... (6 cases)
  gemv_stream<m=4,dual=0,ksplit=4,ku=3,rw=2,wq=bf16>   st_bf16_m3_d0_ks4_ku3_rw2_k4608_rms_mod_gr_inpl
  gemv_stream<m=4,dual=0,ksplit=4,ku=4,rw=2,wq=bf16>   st_bf16_m4_d0_ks4_ku4_rw2_k6656_silu_b
  gemv_stream<m=4,dual=0,ksplit=4,ku=5,rw=2,wq=bf16>   st_bf16_m3_d0_ks4_ku5_rw2_k8704_b_gelu_gc_res, split_m5_k8712_b_gr_res, ... (5 cases)
  gemv_stream<m=4,dual=0,ksplit=8,ku=2,rw=2,wq=bf16>   st_bf16_m4_d0_ks8_ku2_rw2_k6656_b_inpl   [gemv_long_ku]
  gemv_stream<m=4,dual=0,ksplit=8,ku=3,rw=2,wq=bf16>   st_bf16_m3_d0_ks8_ku3_rw2_k10752_rms_gelu_gr
  gemv_stream<m=4,dual=0,ksplit=8,ku=4,rw=2,wq=bf16>   st_bf16_m4_d0_ks8_ku4_rw2_k12800_gc_bcast
  gemv_stream<m=4,dual=0,ksplit=8,ku=5,rw=2,wq=bf16>   st_bf16_m3_d0_ks8_ku5_rw2_k16896_rms_b_res_bcast
  gemv_stream<m=4,dual=0,ksplit=16,ku=2,rw=2,wq=bf16>  st_bf16_m4_d0_ks16_ku2_rw2_k12800_plain   [gemv_long_ku]
  gemv_stream<m=4,dual=0,ksplit=16,ku=3,rw=2,wq=bf16>  st_bf16_m3_d0_ks16_ku3_rw2_k20992_rms_b
  gemv_stream<m=4,dual=0,ksplit=16,ku=4,rw=2,wq=bf16>  st_bf16_m4_d0_ks16_ku4_rw2_k25088_rms_now_res
  gemv_stream<m=4,dual=0,ksplit=16,ku=5,rw=2,wq=bf16>  st_bf16_m3_d0_ks16_ku5_rw2_k33280_rms_mod_gr_inpl
  gemv_stream<m=4,dual=1,ksplit=1,ku=1,rw=1,wq=bf16>   st_bf16_m4_d1_ks1_ku1_rw1_k512_rms_mod_swiglu_gc
  gemv_stream<m=4,dual=1,ksplit=1,ku=1,rw=2,wq=bf16>   st_bf16_m3_d1_ks1_ku1_rw2_k504_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=1,ku=2,rw=1,wq=bf16>   st_bf16_m4_d1_ks1_ku2_rw1_k1024_silu_b_swiglu, split_m5_dual_k520_swiglu_gr_inpl, ... (5 cases)
  gemv_stream<m=4,dual=1,ksplit=1,ku=2,rw=2,wq=bf16>   st_bf16_m3_d1_ks1_ku2_rw2_k1016_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=1,ku=3,rw=1,wq=bf16>   st_bf16_m4_d1_ks1_ku3_rw1_k1536_rms_swiglu
  gemv_stream<m=4,dual=1,ksplit=1,ku=3,rw=2,wq=bf16>   st_bf16_m3_d1_ks1_ku3_rw2_k1528_swiglu_gr_res   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=1,ku=4,rw=1,wq=bf16>   st_bf16_m4_d1_ks1_ku4_rw1_k2048_rms_mod_swiglu_gc, st_waves3_m3_d1_n10, ... (5 cases)
  gemv_stream<m=4,dual=1,ksplit=1,ku=4,rw=2,wq=bf16>   st_bf16_m3_d1_ks1_ku4_rw2_k2040_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=1,ku=5,rw=1,wq=bf16>   st_bf16_m4_d1_ks1_ku5_rw1_k2560_silu_b_swiglu
  gemv_stream<m=4,dual=1,ksplit=1,ku=5,rw=2,wq=bf16>   st_bf16_m3_d1_ks1_ku5_rw2_k2312_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=4,ku=2,rw=1,wq=bf16>   st_bf16_m4_d1_ks4_ku2_rw1_k3064_rms_swiglu
  gemv_stream<m=4,dual=1,ksplit=4,ku=2,rw=2,wq=bf16>   st_bf16_m3_d1_ks4_ku2_rw2_k3072_swiglu_gr_res   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=4,ku=3,rw=1,wq=bf16>   st_bf16_m4_d1_ks4_ku3_rw1_k4600_rms_mod_swiglu_gc
  gemv_stream<m=4,dual=1,ksplit=4,ku=3,rw=2,wq=bf16>   st_bf16_m3_d1_ks4_ku3_rw2_k4608_rms_now_swiglu_inpl   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=8,ku=2,rw=1,wq=bf16>   st_bf16_m4_d1_ks8_ku2_rw1_k6648_silu_b_swiglu
  gemv_stream<m=4,dual=1,ksplit=8,ku=2,rw=2,wq=bf16>   st_bf16_m3_d1_ks8_ku2_rw2_k6656_rms_swiglu_bcast   [gemv_dual_rw]
  gemv_stream<m=4,dual=1,ksplit=8,ku=3,rw=1,wq=bf16>   st_bf16_m4_d1_ks8_ku3_rw1_k8696_rms_swiglu
  gemv_stream<m=4,dual=1,ksplit=8,ku=3,rw=2,wq=bf16>   st_bf16_m3_d1_ks8_ku3_rw2_k8704_swiglu_gr_res   [gemv_dual_rw]
  gemv_stream<m=8,dual=0,ksplit=1,ku=1,rw=1,wq=bf16>   st_m8_5rows_ks1_ku1_b_inpl, st_m8_6rows_ks1_ku1_rms_gelu_gr, ... (4 cases)
  gemv_stream<m=8,dual=0,ksplit=1,ku=2,rw=1,wq=bf16>   st_m8_5rows_ks1_ku2_b_inpl, st_m8_6rows_ks1_ku2_rms_gelu_gr, ... (13 cases)
  gemv_stream<m=8,dual=0,ksplit=4,ku=2,rw=2,wq=bf16>   st_m8_5rows_ks4_ku2_rms_b_res_bcast, st_m8_6rows_ks4_ku2_plain, ... (5 cases)
  gemv_stream<m=8,dual=0,ksplit=8,ku=2,rw=2,wq=bf16>   st_m8_5rows_ks8_ku2_rms_mod_gr_inpl, st_m8_6rows_ks8_ku2_silu_b, ... (4 cases)
  gemv_rows<dual=0,nw=4,ks=3,pers=0,f8=0>              rows_s3, rows_rowmajor_n37_split, ... (4 cases)
  gemv_rows<dual=0,nw=4,ks=6,pers=0,f8=0>              rows_s6, rows_d0_dropped_slice_k2336   [gemv_rows_blocks]
  gemv_rows<dual=0,nw=4,ks=9,pers=0,f8=0>              rows_s9   [gemv_rows_blocks]
  gemv_rows<dual=0,nw=4,ks=12,pers=0,f8=0>             rows_s12
  gemv_rows<dual=0,nw=8,ks=4,pers=0,f8=0>              rows_w4, rows_rowmajor_n37
  gemv_rows<dual=0,nw=8,ks=6,pers=0,f8=0>              rows_w6
  gemv_rows<dual=0,nw=8,ks=8,pers=0,f8=0>              rows_w8
  gemv_rows<dual=1,nw=8,ks=4,pers=0,f8=0>              rows_d_w4, rows_d_s4, ... (3 cases)
  gemv_rows<dual=1,nw=8,ks=6,pers=0,f8=0>              rows_d_w6, rows_d_s6
  gemv_rows<dual=1,nw=8,ks=8,pers=0,f8=0>              rows_d_w8, rows_d_s8
  gemv_rows<dual=1,nw=8,ks=4,pers=1,f8=0>              rows_d_p4_7groups   [gemv_rows_pers]
  gemv_rows<dual=1,nw=8,ks=6,pers=1,f8=0>              rows_d_p6_7groups_ragged   [gemv_rows_pers]
  gemv_rows<dual=0,nw=8,ks=2,pers=0,f8=1>              rows_f8_w2
  gemv_rows<dual=0,nw=8,ks=4,pers=0,f8=1>              rows_f8_w4
  gemv_rows<dual=1,nw=8,ks=2,pers=0,f8=1>              rows_f8_d_w2, rows_f8_d_s2
  gemv_rows<dual=1,nw=8,ks=4,pers=0,f8=1>              rows_f8_d_w4, rows_f8_d_s4
  gemv_rows<dual=1,nw=8,ks=2,pers=1,f8=1>              rows_f8_d_p2_7groups   [gemv_rows_pers]
  gemv_rows<dual=1,nw=8,ks=4,pers=1,f8=1>              rows_f8_d_p4_7groups   [gemv_rows_pers]
  gemv_rows<dual=0,nw=4,ks=2,pers=0,f8=1>              rows_f8_s2, rows_f8_inplace_atomic, ... (3 cases)
  gemv_rows<dual=0,nw=4,ks=4,pers=0,f8=1>              rows_f8_s4   [gemv_rows_blocks]
  gemv_rows<dual=0,nw=4,ks=6,pers=0,f8=1>              rows_f8_s6   [gemv_rows_blocks]
  gemv_rows<dual=0,nw=4,ks=8,pers=0,f8=1>              rows_f8_s8
  gemv_lds<w=f32,m=1,dual=0,ks=4,np=2>                 lds_f32_m1_d0_ks4_np2_n1026_k2056_rms_now_res
  gemv_lds<w=f32,m=1,dual=0,ks=4,np=1>                 lds_f32_m1_d0_ks4_np1_n3_k2048_rms_mod_gr_inpl
  gemv_lds<w=f32,m=1,dual=0,ks=1,np=2>                 lds_f32_m1_d0_ks1_np2_n8193_k24_silu_b
  gemv_lds<w=f32,m=1,dual=0,ks=1,np=1>                 lds_f32_m1_d0_ks1_np1_n7_k520_b_gelu_gc_res
  gemv_lds<w=f32,m=1,dual=1,ks=4,np=2>                 lds_f32_m1_d1_ks4_np2_n1026_k2056_rms_swiglu
  gemv_lds<w=f32,m=1,dual=1,ks=4,np=1>                 lds_f32_m1_d1_ks4_np1_n2_k2056_swiglu_gr_res
  gemv_lds<w=f32,m=1,dual=1,ks=1,np=2>                 lds_f32_m1_d1_ks1_np2_n8193_k24_rms_mod_swiglu_gc
  gemv_lds<w=f32,m=1,dual=1,ks=1,np=1>                 lds_f32_m1_d1_ks1_np1_n5_k520_rms_now_swiglu_inpl
  gemv_lds<w=f32,m=2,dual=0,ks=4,np=2>                 lds_f32_m2_d0_ks4_np2_n1026_k2056_plain
  gemv_lds<w=f32,m=2,dual=0,ks=4,np=1>                 lds_f32_m2_d0_ks4_np1_n1_k2064_rms_b
  gemv_lds<w=f32,m=2,dual=0,ks=1,np=2>                 lds_f32_m2_d0_ks1_np2_n8193_k24_rms_now_res
  gemv_lds<w=f32,m=2,dual=0,ks=1,np=1>                 lds_f32_m2_d0_ks1_np1_n3_k520_rms_mod_gr_inpl
  gemv_lds<w=f32,m=2,dual=1,ks=4,np=2>                 lds_f32_m2_d1_ks4_np2_n1026_k2056_rms_mod_swiglu_gc
  gemv_lds<w=f32,m=2,dual=1,ks=4,np=1>                 lds_f32_m2_d1_ks4_np1_n7_k2048_rms_now_swiglu_inpl
  gemv_lds<w=f32,m=2,dual=1,ks=1,np=2>                 lds_f32_m2_d1_ks1_np2_n8193_k24_silu_b_swiglu
  gemv_lds<w=f32,m=2,dual=1,ks=1,np=1>                 lds_f32_m2_d1_ks1_np1_n2_k520_rms_swiglu_bcast
  gemv_lds<w=f32,m=3,dual=0,ks=4,np=2>                 lds_f32_m3_d0_ks4_np2_n1026_k2056_gc_bcast
  gemv_lds<w=f32,m=3,dual=0,ks=4,np=1>                 lds_f32_m3_d0_ks4_np1_n5_k2056_rms_b_res_bcast
  gemv_lds<w=f32,m=3,dual=0,ks=1,np=2>                 lds_f32_m3_d0_ks1_np2_n8193_k24_plain
  gemv_lds<w=f32,m=3,dual=0,ks=1,np=1>                 lds_f32_m3_d0_ks1_np1_n1_k520_rms_b
  gemv_lds<w=f32,m=3,dual=1,ks=4,np=2>                 lds_f32_m3_d1_ks4_np2_n1026_k2056_silu_b_swiglu
  gemv_lds<w=f32,m=3,dual=1,ks=4,np=1>                 lds_f32_m3_d1_ks4_np1_n3_k2064_rms_swiglu_bcast
  gemv_lds<w=f32,m=3,dual=1,ks=1,np=1>                 lds_f32_m3_d1_ks1_np1_n41_k520_rms_swiglu
  gemv_lds<w=f32,m=4,dual=0,ks=4,np=2>                 lds_f32_m4_d0_ks4_np2_n1026_k2056_b_gelu_gc_res
  gemv_lds<w=f32,m=4,dual=0,ks=4,np=1>                 lds_f32_m4_d0_ks4_np1_n50_k2064_b_inpl
  gemv_lds<w=f32,m=4,dual=0,ks=1,np=2>                 lds_f32_m4_d0_ks1_np2_n8193_k24_rms_gelu_gr
  gemv_lds<w=f32,m=4,dual=0,ks=1,np=1>                 lds_f32_m4_d0_ks1_np1_n45_k520_gc_bcast
  gemv_lds<w=f32,m=4,dual=1,ks=4,np=2>                 lds_f32_m4_d1_ks4_np2_n1026_k2056_rms_swiglu_bcast
  gemv_lds<w=f32,m=4,dual=1,ks=4,np=1>                 lds_f32_m4_d1_ks4_np1_n37_k2048_rms_swiglu
  gemv_lds<w=f32,m=4,dual=1,ks=1,np=1>                 lds_f32_m4_d1_ks1_np1_n1_k520_swiglu_gr_res
  gemv_lds<w=f32,m=5,dual=0,ks=4,np=2>                 lds_f32_m5_d0_ks4_np2_n1026_k2056_plain
  gemv_lds<w=f32,m=5,dual=0,ks=4,np=1>                 lds_f32_m5_d0_ks4_np1_n3_k2048_rms_b
  gemv_lds<w=f32,m=5,dual=0,ks=1,np=1>                 lds_f32_m5_d0_ks1_np1_n41_k520_rms_now_res
  gemv_lds<w=f32,m=5,dual=1,ks=4,np=2>                 lds_f32_m5_d1_ks4_np2_n1026_k2056_rms_swiglu
  gemv_lds<w=f32,m=5,dual=1,ks=4,np=1>                 lds_f32_m5_d1_ks4_np1_n50_k2048_swiglu_gr_res
  gemv_lds<w=f32,m=5,dual=1,ks=1,np=1>                 lds_f32_m5_d1_ks1_np1_n2_k520_rms_mod_swiglu_gc
  gemv_lds<w=f32,m=6,dual=0,ks=4,np=2>                 lds_f32_m6_d0_ks4_np2_n1026_k2056_b_inpl
  gemv_lds<w=f32,m=6,dual=0,ks=4,np=1>                 lds_f32_m6_d0_ks4_np1_n5_k2048_rms_gelu_gr
  gemv_lds<w=f32,m=6,dual=0,ks=1,np=1>                 lds_f32_m6_d0_ks1_np1_n37_k520_plain
  gemv_lds<w=f32,m=6,dual=1,ks=4,np=2>                 lds_f32_m6_d1_ks4_np2_n1026_k2056_swiglu_gr_res
  gemv_lds<w=f32,m=6,dual=1,ks=4,np=1>                 lds_f32_m6_d1_ks4_np1_n33_k2048_rms_mod_swiglu_gc
  gemv_lds<w=f32,m=6,dual=1,ks=1,np=1>                 lds_f32_m6_d1_ks1_np1_n3_k520_rms_now_swiglu_inpl
  gemv_lds<w=f32,m=7,dual=0,ks=4,np=2>                 lds_f32_m7_d0_ks4_np2_n1026_k2056_silu_b
  gemv_lds<w=f32,m=7,dual=0,ks=4,np=1>                 lds_f32_m7_d0_ks4_np1_n7_k2048_b_gelu_gc_res
  gemv_lds<w=f32,m=7,dual=0,ks=1,np=1>                 lds_f32_m7_d0_ks1_np1_n50_k520_b_inpl
  gemv_lds<w=f32,m=7,dual=1,ks=4,np=2>                 lds_f32_m7_d1_ks4_np2_n1026_k2056_rms_mod_swiglu_gc
  gemv_lds<w=f32,m=7,dual=1,ks=4,np=1>                 lds_f32_m7_d1_ks4_np1_n45_k2048_rms_now_swiglu_inpl
  gemv_lds<w=f32,m=7,dual=1,ks=1,np=1>                 lds_f32_m7_d1_ks1_np1_n5_k520_silu_b_swiglu
  gemv_lds<w=f32,m=8,dual=0,ks=4,np=2>                 lds_f32_m8_d0_ks4_np2_n1026_k2056_rms_now_res
  gemv_lds<w=f32,m=8,dual=0,ks=4,np=1>                 lds_f32_m8_d0_ks4_np1_n1_k2048_rms_mod_gr_inpl, lds_f32_m8_two_chunks_k2056
  gemv_lds<w=f32,m=8,dual=0,ks=1,np=1>                 lds_f32_m8_d0_ks1_np1_n33_k1032_silu_b
  gemv_lds<w=f32,m=8,dual=1,ks=4,np=2>                 lds_f32_m8_d1_ks4_np2_n1026_k2056_rms_now_swiglu_inpl
  gemv_lds<w=f32,m=8,dual=1,ks=4,np=1>                 lds_f32_m8_d1_ks4_np1_n41_k2048_silu_b_swiglu
  gemv_lds<w=f32,m=8,dual=1,ks=1,np=1>                 lds_f32_m8_d1_ks1_np1_n7_k1032_rms_swiglu
  gemv_lds<w=bf16,m=1,dual=0,ks=4,np=2>                lds_bf16_m1_d0_ks4_np2_n1026_k2056_b_inpl
  gemv_lds<w=bf16,m=1,dual=0,ks=4,np=1>                lds_bf16_m1_d0_ks4_np1_n2_k2048_rms_gelu_gr
  gemv_lds<w=bf16,m=1,dual=0,ks=1,np=2>                lds_bf16_m1_d0_ks1_np2_n8193_k24_gc_bcast
  gemv_lds<w=bf16,m=1,dual=0,ks=1,np=1>                lds_bf16_m1_d0_ks1_np1_n5_k520_rms_b_res_bcast
  gemv_lds<w=bf16,m=1,dual=1,ks=4,np=2>                lds_bf16_m1_d1_ks4_np2_n1026_k2056_rms_swiglu
  gemv_lds<w=bf16,m=1,dual=1,ks=4,np=1>                lds_bf16_m1_d1_ks4_np1_n1_k2056_rms_now_swiglu_inpl
  gemv_lds<w=bf16,m=1,dual=1,ks=1,np=2>                lds_bf16_m1_d1_ks1_np2_n8193_k24_rms_mod_swiglu_gc
  gemv_lds<w=bf16,m=1,dual=1,ks=1,np=1>                lds_bf16_m1_d1_ks1_np1_n3_k520_rms_now_swiglu_inpl
  gemv_lds<w=bf16,m=2,dual=0,ks=4,np=2>                lds_bf16_m2_d0_ks4_np2_n1026_k2056_silu_b
  gemv_lds<w=bf16,m=2,dual=0,ks=4,np=1>                lds_bf16_m2_d0_ks4_np1_n7_k2064_b_gelu_gc_res
  gemv_lds<w=bf16,m=2,dual=0,ks=1,np=2>                lds_bf16_m2_d0_ks1_np2_n8193_k24_b_inpl
  gemv_lds<w=bf16,m=2,dual=0,ks=1,np=1>                lds_bf16_m2_d0_ks1_np1_n2_k520_rms_gelu_gr
  gemv_lds<w=bf16,m=2,dual=1,ks=4,np=2>                lds_bf16_m2_d1_ks4_np2_n1026_k2056_rms_mod_swiglu_gc
  gemv_lds<w=bf16,m=2,dual=1,ks=4,np=1>                lds_bf16_m2_d1_ks4_np1_n5_k2048_rms_now_swiglu_inpl
  gemv_lds<w=bf16,m=2,dual=1,ks=1,np=2>                lds_bf16_m2_d1_ks1_np2_n8193_k24_silu_b_swiglu
  gemv_lds<w=bf16,m=2,dual=1,ks=1,np=1>                lds_bf16_m2_d1_ks1_np1_n1_k520_rms_swiglu_bcast
  gemv_lds<w=bf16,m=3,dual=0,ks=4,np=2>                lds_bf16_m3_d0_ks4_np2_n1026_k2056_rms_now_res
  gemv_lds<w=bf16,m=3,dual=0,ks=4,np=1>                lds_bf16_m3_d0_ks4_np1_n3_k2056_rms_mod_gr_inpl
  gemv_lds<w=bf16,m=3,dual=0,ks=1,np=2>                lds_bf16_m3_d0_ks1_np2_n8193_k24_silu_b
  gemv_lds<w=bf16,m=3,dual=0,ks=1,np=1>                lds_bf16_m3_d0_ks1_np1_n7_k520_b_gelu_gc_res
  gemv_lds<w=bf16,m=3,dual=1,ks=4,np=2>                lds_bf16_m3_d1_ks4_np2_n1026_k2056_silu_b_swiglu
  gemv_lds<w=bf16,m=3,dual=1,ks=4,np=1>                lds_bf16_m3_d1_ks4_np1_n2_k2064_rms_swiglu_bcast
  gemv_lds<w=bf16,m=3,dual=1,ks=1,np=1>                lds_bf16_m3_d1_ks1_np1_n45_k520_rms_swiglu
  gemv_lds<w=bf16,m=4,dual=0,ks=4,np=2>                lds_bf16_m4_d0_ks4_np2_n1026_k2056_rms_b_res_bcast
  gemv_lds<w=bf16,m=4,dual=0,ks=4,np=1>                lds_bf16_m4_d0_ks4_np1_n37_k2064_plain
  gemv_lds<w=bf16,m=4,dual=0,ks=1,np=2>                lds_bf16_m4_d0_ks1_np2_n8193_k24_rms_b
  gemv_lds<w=bf16,m=4,dual=0,ks=1,np=1>                lds_bf16_m4_d0_ks1_np1_n33_k520_rms_now_res
  gemv_lds<w=bf16,m=4,dual=1,ks=4,np=2>                lds_bf16_m4_d1_ks4_np2_n1026_k2056_rms_swiglu_bcast
  gemv_lds<w=bf16,m=4,dual=1,ks=4,np=1>                lds_bf16_m4_d1_ks4_np1_n41_k2048_rms_swiglu
  gemv_lds<w=bf16,m=4,dual=1,ks=1,np=1>                lds_bf16_m4_d1_ks1_np1_n7_k520_swiglu_gr_res
  gemv_lds<w=bf16,m=5,dual=0,ks=4,np=2>                lds_bf16_m5_d0_ks4_np2_n1026_k2056_b_inpl
  gemv_lds<w=bf16,m=5,dual=0,ks=4,np=1>                lds_bf16_m5_d0_ks4_np1_n2_k2048_rms_gelu_gr
  gemv_lds<w=bf16,m=5,dual=0,ks=1,np=1>                lds_bf16_m5_d0_ks1_np1_n45_k520_plain
  gemv_lds<w=bf16,m=5,dual=1,ks=4,np=2>                lds_bf16_m5_d1_ks4_np2_n1026_k2056_silu_b_swiglu
  gemv_lds<w=bf16,m=5,dual=1,ks=4,np=1>                lds_bf16_m5_d1_ks4_np1_n37_k2048_rms_swiglu
  gemv_lds<w=bf16,m=5,dual=1,ks=1,np=1>                lds_bf16_m5_d1_ks1_np1_n1_k520_swiglu_gr_res
  gemv_lds<w=bf16,m=6,dual=0,ks=4,np=2>                lds_bf16_m6_d0_ks4_np2_n1026_k2056_silu_b
  gemv_lds<w=bf16,m=6,dual=0,ks=4,np=1>                lds_bf16_m6_d0_ks4_np1_n3_k2048_b_gelu_gc_res
  gemv_lds<w=bf16,m=6,dual=0,ks=1,np=1>                lds_bf16_m6_d0_ks1_np1_n41_k520_b_inpl
  gemv_lds<w=bf16,m=6,dual=1,ks=4,np=2>                lds_bf16_m6_d1_ks4_np2_n1026_k2056_rms_swiglu
  gemv_lds<w=bf16,m=6,dual=1,ks=4,np=1>                lds_bf16_m6_d1_ks4_np1_n50_k2048_swiglu_gr_res
  gemv_lds<w=bf16,m=6,dual=1,ks=1,np=1>                lds_bf16_m6_d1_ks1_np1_n2_k520_rms_mod_swiglu_gc
  gemv_lds<w=bf16,m=7,dual=0,ks=4,np=2>                lds_bf16_m7_d0_ks4_np2_n1026_k2056_rms_now_res
  gemv_lds<w=bf16,m=7,dual=0,ks=4,np=1>                lds_bf16_m7_d0_ks4_np1_n5_k2048_rms_mod_gr_inpl
  gemv_lds<w=bf16,m=7,dual=0,ks=1,np=1>                lds_bf16_m7_d0_ks1_np1_n37_k520_silu_b
  gemv_lds<w=bf16,m=7,dual=1,ks=4,np=2>                lds_bf16_m7_d1_ks4_np2_n1026_k2056_swiglu_gr_res
  gemv_lds<w=bf16,m=7,dual=1,ks=4,np=1>                lds_bf16_m7_d1_ks4_np1_n33_k2048_rms_mod_swiglu_gc
  gemv_lds<w=bf16,m=7,dual=1,ks=1,np=1>                lds_bf16_m7_d1_ks1_np1_n3_k520_rms_now_swiglu_inpl
  gemv_lds<w=bf16,m=8,dual=0,ks=4,np=2>                lds_bf16_m8_d0_ks4_np2_n1026_k2056_plain
  gemv_lds<w=bf16,m=8,dual=0,ks=4,np=1>                lds_bf16_m8_d0_ks4_np1_n7_k2048_rms_b
  gemv_lds<w=bf16,m=8,dual=0,ks=1,np=1>                lds_bf16_m8_d0_ks1_np1_n50_k1032_rms_now_res
  gemv_lds<w=bf16,m=8,dual=1,ks=4,np=2>                lds_bf16_m8_d1_ks4_np2_n1026_k2056_rms_mod_swiglu_gc
  gemv_lds<w=bf16,m=8,dual=1,ks=4,np=1>                lds_bf16_m8_d1_ks4_np1_n45_k2048_rms_now_swiglu_inpl
  gemv_lds<w=bf16,m=8,dual=1,ks=1,np=1>                lds_bf16_m8_d1_ks1_np1_n5_k1032_silu_b_swiglu
  gemv_generic<w=f32>                                  gen_f32_m1_k13_plain, gen_f32_m3_k100_rms_now_res, ... (4 cases)
  gemv_generic<w=bf16>                                 gen_bf16_m2_k13_swiglu_gr_res, gen_bf16_m8_k1001_rms_now_swiglu_inpl, ... (4 cases)
"""
import ctypes as C
import functools
import itertools
import math
import os
import sys
import zlib

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_rms
from test_hip_mfma_gemm import NAN, _FAKE, _epilogue, _gapped, _lib, _need_gpu, _prologue, _same_bits, bf16_round64, built_kernels, instantiations_of

EPS = 1e-5

# One constant per route class, held for the global, the worst-row and the worst-element figure alike.  Chosen from the arithmetic, then checked
# against both conditions on the CPU (test_bars_sit_between_floor_and_dropped_chunk); never from what the device gives.  Every weight type here
# (bf16, fp8 code x power-of-two scale, NF4 table x absmax rounded to bf16, fp32) is exact in fp32 and in the reference, so the classes differ by
# the prologue and by whether the operands pass through the matrix cores, not by the weight type.
#   none      VALU kernels, no prologue: fp32 products and sums alone.  A sum of K terms taken in 8-column chunks one after the other carries
#             ~ 2^-24 sqrt(K / 8 / 2) of its own rms: 1.7e-6 at the longest K here (40960); the worst of ~ 400 elements is ~ 3.5 sigma and a
#             per-row gate of up to 3 multiplies it: ~ 2e-5, times the 8 x headroom 1.6e-4.  The cheapest dropped chunk (K = 40960) costs
#             sqrt(8 / 40960) = 1.4e-2, so the bar may not pass 1.4e-3: 3e-4.
#   rms       the same sum behind x rsqrt(mean x^2 + eps) [* w]: three more fp32 roundings per activation (2^-24 each, they average out over K)
#             and one rsqrtf per row (<= 2 ulp, common to the row: 1.2e-7 of every element) - nothing next to the sum's own error: 3e-4.
#   rms_mod   two more fp32 operations, x (1 + scale) + shift: 3e-4.
#   silu      expf and a division per activation (<= 2 ulp each): 3e-4.  K <= 2568 in this class.
#   rows      matrix cores: each activation enters as bf16 hi + bf16 lo, 2^-17 of its value at worst, in the reference too - but the device's
#             fp32 prologue (and, split over K, its un-normalised slices) can put hi / lo one step off the reference's: up to 2^-17 per product,
#             2^-17 / sqrt(3) = 4.4e-6 of an output's rms, 3.5 sigma over ~ 400 elements and a gate of 3: 5e-5, on top of the fp32 sum as above
#             (K <= 8256 here: 8e-6), and times the 8 x headroom 4e-4.  3e-4, as the VALU classes: the fp32 stand-in, whose hi / lo pairs come
#             from its own fp32 prologue, sits at 2e-5 for its worst element.  The cheapest dropped chunk of the class costs sqrt(8 / 8256) = 3.1e-2.
#   rows_rms  the same with the RMSNorm prologue in front (and rstd applied after the product in the split-K forms): 3e-4.
BAR = {"none": 3e-4, "rms": 3e-4, "rms_mod": 3e-4, "silu": 3e-4, "rows": 3e-4, "rows_rms": 3e-4}
FLOOR_HEADROOM = 8.0
DROP_MARGIN = 10.0

TUNE_DEFAULTS = {"gemv_small_rw": 2, "gemv_dual_rw": 1, "gemv_long_ku": 5, "gemv_rows_pers": 192, "gemv_rows_blocks": 448, "gemv_rows_atomic": 1,
                 "gemv_rows_scratch": 0, "gemv_opt": 13, "gemv_waves": 0, "gemv_blocks": 0}
WQS = ("bf16", "fp8", "nf4")


# ---------------------------------------------------------------------------------------------------------------
# the launch ladders' rules, restated: names, the compiled set, the decisions
# ---------------------------------------------------------------------------------------------------------------
def _stream(m, dual, ksplit, ku, rw, wq):
    return f"gemv_stream<m={m},dual={dual},ksplit={ksplit},ku={ku},rw={rw},wq={wq}>"


def _rows(dual, nw, ks, pers, f8):
    return f"gemv_rows<dual={dual},nw={nw},ks={ks},pers={pers},f8={f8}>"


def _lds(w, m, dual, ks, np_):
    return f"gemv_lds<w={w},m={m},dual={dual},ks={ks},np={np_}>"


def stream_built(dual, ksplit, ku):
    """(dual, ksplit, ku) forms of the M = 1 / 2 / 4 streaming kernels the ladder instantiates"""
    if ksplit not in (1, 4, 8, 16) or not 1 <= ku <= 5 or (ku == 1 and ksplit != 1):
        return False
    return not (dual and (ksplit == 16 or (ksplit != 1 and ku > 3)))


def stream_built_nf4(m, dual, ksplit, ku):
    return stream_built(dual, ksplit, ku) and m <= 2 and ksplit <= 8 and not (dual and ku > 4)


M8_FORMS = [(1, 1, 1), (1, 2, 1), (4, 2, 2), (8, 2, 2)]            # (ksplit, ku, rw)
ROWS_FORMS = [(0, 4, 3, 0, 0), (0, 4, 6, 0, 0), (0, 4, 9, 0, 0), (0, 4, 12, 0, 0), (0, 8, 4, 0, 0), (0, 8, 6, 0, 0), (0, 8, 8, 0, 0),
              (1, 8, 4, 0, 0), (1, 8, 6, 0, 0), (1, 8, 8, 0, 0), (1, 8, 4, 1, 0), (1, 8, 6, 1, 0),
              (0, 8, 2, 0, 1), (0, 8, 4, 0, 1), (1, 8, 2, 0, 1), (1, 8, 4, 0, 1), (1, 8, 2, 1, 1), (1, 8, 4, 1, 1),
              (0, 4, 2, 0, 1), (0, 4, 4, 0, 1), (0, 4, 6, 0, 1), (0, 4, 8, 0, 1)]


def stream_exists(m, dual, ksplit, ku, rw, wq):
    """stream_exists of vv_gemv_stream.hip: the kernels the launch ladder instantiates"""
    if m == 8:
        return wq == "bf16" and not dual and (ksplit, ku, rw) in M8_FORMS
    if m not in (1, 2, 4):
        return False
    if wq == "nf4":
        return rw == 4 and stream_built_nf4(m, dual, ksplit, ku)
    if wq == "fp8" and m > 2:
        return False
    if rw not in (1, 2) or (rw == 1 and not dual and ksplit != 1):
        return False
    return stream_built(dual, ksplit, ku)


def lds_built(m, dual, ks, np_):
    """lds_built of vv_kernels.hip: two whole rows per wave (ks = 1, np = 2) exist for m <= 4 (dual: m <= 2) only"""
    return ks == 4 or np_ == 1 or (m <= 4 and not (dual and m > 2))


def _compiled():
    """Every instantiation the launch ladders compile, by their predicates: what is compiled is what a call can reach, under default tuning or
    under a vv_tune setting (test_built_library_holds_exactly_the_enumerated_kernels reads the binary)."""
    out = [_stream(m, dual, ksplit, ku, rw, wq) for m in (1, 2, 4) for dual, ksplit, ku in itertools.product((0, 1), (1, 4, 8, 16), range(1, 6))
           for rw in (1, 2, 4) for wq in WQS if stream_exists(m, dual, ksplit, ku, rw, wq)]
    out += [_stream(8, 0, ks, ku, rw, "bf16") for ks, ku, rw in M8_FORMS]
    out += [_rows(*f) for f in ROWS_FORMS]
    out += [_lds(w, m, dual, ks, np_) for w in ("f32", "bf16") for m in range(1, 9) for dual in (0, 1) for ks, np_ in ((4, 2), (4, 1), (1, 2), (1, 1))
            if lds_built(m, dual, ks, np_)]
    out += ["gemv_generic<w=f32>", "gemv_generic<w=bf16>"]
    return out


ALL_INSTANTIATIONS = _compiled()


def stream_decide(m, n, k, dual, wq, tune):
    """vv_gemv_stream_decide for aligned operands and no hot-table shape: the instantiation name, or None (not covered)"""
    if k % 8 or m > 8 or (wq != "bf16" and m > 2) or (wq == "nf4" and k % 64):
        return None
    units = -(-k // 512)
    if m > 4:
        if dual:
            return None
        for w in (1, 4, 8):
            if -(-units // w) <= 2:
                return _stream(8, 0, w, -(-units // w) if w == 1 else 2, 1 if w == 1 else 2, "bf16")
        return None
    ksplit, ku = 1, units
    if units > (4 if (wq == "nf4" and dual) else 5):
        kumax = 3 if dual else (tune.get("gemv_long_ku", 5) if units > 12 else 5)
        ksplit = next((w for w in (4, 8, 16) if -(-units // w) <= kumax), 0)
        if not ksplit:
            return None
        ku = max(2, -(-units // ksplit))
    mt = 4 if m > 2 else m
    if wq == "nf4":
        return _stream(mt, dual, ksplit, ku, 4, wq) if stream_built_nf4(mt, dual, ksplit, ku) else None
    if not stream_built(dual, ksplit, ku):
        return None
    if dual:
        rw = 1 if tune.get("gemv_dual_rw", 1) == 1 else 2
    else:
        rw = 1 if (ksplit == 1 and n <= 4096 and tune.get("gemv_small_rw", 2) == 1) else 2
    return _stream(mt, dual, ksplit, ku, rw, wq)


def rows_decide(m, n, k, dual, f8, mod, atomic_ok, tune):
    """vv_gemv_rows_decide with the process-wide scratch on, aligned operands: (instantiation, ksplit before the drop, ksplit, atomic) or None"""
    pers_cap, blocks = tune.get("gemv_rows_pers", 192), tune.get("gemv_rows_blocks", 448)
    wide = 64 if f8 else 32
    if not 3 <= m <= 8 or k % wide or k < 32 or (f8 and n % 16):
        return None
    steps, groups = k // wide, -(-n // 16)
    if steps <= (32 if f8 else 64):
        spw = -(-steps // 8)
        if f8:
            return _rows(dual, 8, 2 if spw <= 2 else 4, int(bool(dual) and groups > pers_cap), 1), 1, 1, 0
        ks = 4 if spw <= 4 else 6 if spw <= 6 else 8
        return _rows(dual, 8, ks, int(bool(dual) and groups > pers_cap and spw <= 6), 0), 1, 1, 0
    if mod:
        return None
    nw = 8 if dual else 4
    kscap, ksmax, small = ((4, 4, 2) if dual else (6, 8, 2)) if f8 else ((8, 8, 3) if dual else (9, 12, 3))
    pick = next(((sp, -(-steps // (sp * nw))) for sp in range(2, 17)
                 if -(-steps // (sp * nw)) <= kscap and (groups * sp >= blocks or -(-steps // (sp * nw)) <= small)), None)
    if not pick:
        pick = next(((sp, -(-steps // (sp * nw))) for sp in range(2, 17) if -(-steps // (sp * nw)) <= ksmax), None)
    if not pick:
        return None
    ks0, spw = pick
    ksplit = ks0
    while ksplit > 1 and (ksplit - 1) * nw * spw >= steps:
        ksplit -= 1
    atomic = int(bool(tune.get("gemv_rows_atomic", 1)) and not dual and atomic_ok)
    sizes = ((2, 4) if dual else (2, 4, 6, 8)) if f8 else ((4, 6, 8) if dual else (3, 6, 9, 12))
    return _rows(dual, nw, next(s for s in sizes if spw <= s), 0, int(f8)), ks0, ksplit, atomic


def lds_decide(w, m, n, k, dual):
    if n < 4096 and k >= 2048:
        return _lds(w, m, dual, 4, 2 if n >= 1024 else 1)
    return _lds(w, m, dual, 1, 2 if (n >= 8192 and m <= 4 and not (dual and m > 2)) else 1)


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """One vv_linear call.  wq: bf16 | fp8 | nf4 | f32; pro: none | rms (weight) | rms_now (no weight) | silu; mod: adaLN shift / scale from one
    [m, 3k] array; gate: None | "chan" (gate_ld 0) | "row" (third block of a [m, 3n] array); res: None | "out" (its own array, ldres = n + 4) |
    "inplace" (res == out); ldx: None (k + 8) | 0 (one broadcast row) | "k+2" (rows off the 16-byte grid: the streaming kernel declines);
    xoff: x 4 bytes past a 16-byte boundary; woff: w 2 bytes past one; frag: fragment-major weights (rows route)."""

    def __init__(self, cid, route, m, n, k, wq="bf16", pro="none", mod=False, bias=False, act="none", gate=None, res=None, ldx=None, xoff=False,
                 woff=False, frag=False, hooks=None, suffix="", runs=2):
        self.id, self.route, self.m, self.n, self.k, self.wq, self.pro, self.mod, self.bias, self.act = cid, route, m, n, k, wq, pro, mod, bias, act
        self.gate, self.res, self.ldx, self.xoff, self.woff, self.frag, self.hooks = gate, res, ldx, xoff, woff, frag, dict(hooks or {})
        self.suffix, self.runs = suffix, runs            # suffix: what follows the instantiation in the reported name (rows: ksplit / atomic)
        self.dual = int(act == "swiglu")
        self.on_rows = route.startswith("gemv_rows")
        assert not (mod and not pro.startswith("rms"))

    @property
    def name(self):
        return self.route + self.suffix

    @property
    def klass(self):
        if self.on_rows:
            return "rows" if self.pro == "none" else "rows_rms"
        return {"none": "none", "silu": "silu"}.get(self.pro, "rms_mod" if self.mod else "rms")

    @property
    def data_key(self):      # everything the VALUES depend on: layout and tune hooks are not part of it
        return (self.m, self.n, self.k, self.wq, self.pro, self.mod, self.bias, self.act, self.gate, bool(self.res), self.ldx == 0, self.on_rows)


# operand sets, spread over the cases so that each route sees several (dual kernels take the SwiGLU ones)
OPS = [dict(), dict(pro="rms", bias=True), dict(pro="rms_now", res="out"), dict(pro="rms", mod=True, gate="row", res="inplace"),
       dict(pro="silu", bias=True), dict(bias=True, act="gelu", gate="chan", res="out"), dict(bias=True, res="inplace"),
       dict(pro="rms", act="gelu", gate="row"), dict(gate="chan", ldx=0), dict(pro="rms", bias=True, ldx=0, res="out")]
OPS_DUAL = [dict(pro="rms", act="swiglu"), dict(act="swiglu", gate="row", res="out"), dict(pro="rms", mod=True, act="swiglu", gate="chan"),
            dict(pro="rms_now", act="swiglu", res="inplace"), dict(pro="silu", act="swiglu", bias=True), dict(pro="rms", act="swiglu", ldx=0)]
NS = [37, 1, 33, 3, 41, 7, 50, 2, 45, 5]                 # n = 1, odd, not a multiple of rw (2 or 4), below the block's 4 waves
TAILS = {"bf16": (8, 264, 504), "fp8": (16, 272, 496), "nf4": (64, 256, 448), "f32": (8, 264, 504)}


def _cases():
    cs, count = [], itertools.count()

    def add(cid, route, m, n, k, **kw):
        cs.append(Case(cid, route, m, n, k, **kw))

    def ops(dual, i, keep=lambda o: True):
        pool = [o for o in (OPS_DUAL if dual else OPS) if keep(o)]
        return dict(pool[i % len(pool)])

    def one_output(o):
        """m = n = 1: the whole output is one number and its gate one normal draw that scales every error and every dropped chunk alike - there
        is no rms for the bar guard to stand on, so the single-output cases take the operand sets without a gate"""
        return not o.get("gate")

    def tag(o):
        return "_".join(filter(None, [o.get("pro", ""), "mod" if o.get("mod") else "", "b" if o.get("bias") else "", o.get("act", ""),
                                      {"chan": "gc", "row": "gr"}.get(o.get("gate"), ""), {"out": "res", "inplace": "inpl"}.get(o.get("res"), ""),
                                      "bcast" if o.get("ldx") == 0 else ""])) or "plain"

    # ---- streaming kernel: every instantiation once, the smallest k that selects it; whole units and ragged ends alternate -----------------
    reach = {}                                            # instantiation -> (units, hooks)
    for wq, m, dual in itertools.product(WQS, (1, 2, 4), (0, 1)):
        if wq != "bf16" and m > 2:
            continue
        for lk, rwh in itertools.product((5, 3, 2), (0, 1)):
            hooks = {}
            if lk != 5:
                hooks["gemv_long_ku"] = lk
            if rwh:
                hooks["gemv_dual_rw" if dual else "gemv_small_rw"] = 2 if dual else 1
            for units in range(1, 81):
                inst = stream_decide(m, 33, units * 512, dual, wq, hooks)
                if inst and (inst not in reach or len(hooks) < len(reach[inst][1])):
                    reach[inst] = (units, hooks)
    ragged = {}                                           # (ksplit, ku) -> how many cases so far: even = whole units, odd = ragged
    for inst in ALL_INSTANTIATIONS:
        if inst not in reach:
            continue
        units, hooks = reach[inst]
        f = dict(p.split("=") for p in inst[12:-1].split(","))
        wq, mt, dual, key = f["wq"], int(f["m"]), int(f["dual"]), (f["ksplit"], f["ku"])
        i = next(count)
        r = ragged[key] = ragged.get(key, -1) + 1
        k = units * 512 if r % 2 == 0 else (units - 1) * 512 + TAILS[wq][(r // 2) % 3]
        m = 3 if (mt == 4 and i % 2) else mt              # m = 3: a masked fourth row of the M = 4 kernel
        n = NS[i % len(NS)]
        o = ops(dual, i, one_output if m * n == 1 else lambda o: True)
        add(f"st_{wq}_m{m}_d{dual}_ks{f['ksplit']}_ku{f['ku']}_rw{f['rw']}_k{k}_{tag(o)}", inst, m, n, k, wq=wq, hooks=hooks, **o)
    # the unit boundaries themselves, the last wave's slice a single partial unit, a wave with no unit at all
    for i, k in enumerate((8, 504, 512, 520, 2560, 2568)):
        for m, dual in ((1, 0), (2, 1), (3, 0)):
            o = ops(dual, i + m)
            add(f"st_edge_m{m}_d{dual}_k{k}_{tag(o)}", stream_decide(m, 35, k, dual, "bf16", {}), m, 35, k, **o)
    for k, what in ((12 * 512 + 8, "lastpartial"), (9 * 512, "ks4_ku3_wave1_idle"), (21 * 512 - 248, "ks8_lastpartial"), (41 * 512 + 264, "ks16_lastpartial"),
                    (17 * 512, "ks8_ku3_7idle")):
        o = ops(0, k)
        add(f"st_{what}_k{k}_{tag(o)}", stream_decide(2, 35, k, 0, "bf16", {}), 2, 35, k, **o)
    add("st_ks16_waves_13_to_15_no_unit", _stream(1, 0, 16, 2, 2, "bf16"), 1, 35, 13 * 512, pro="rms", bias=True, hooks={"gemv_long_ku": 1})
    assert stream_decide(1, 35, 13 * 512, 0, "bf16", {"gemv_long_ku": 1}) == _stream(1, 0, 16, 2, 2, "bf16")
    add("st_nf4_dual_5units", stream_decide(2, 34, 5 * 512 - 64, 1, "nf4", {}), 2, 34, 5 * 512 - 64, wq="nf4", pro="rms", act="swiglu")
    # 5..8 rows: the four M = 8 forms, each at every row count
    for (ksp, ku, rw), m in itertools.product(M8_FORMS, (5, 6, 7, 8)):
        k = {(1, 1): 504, (1, 2): 1024, (4, 2): 2568, (8, 2): 8192}[(ksp, ku)]
        o = ops(0, m + ksp, lambda o: o.get("act") != "swiglu")
        add(f"st_m8_{m}rows_ks{ksp}_ku{ku}_{tag(o)}", _stream(8, 0, ksp, ku, rw, "bf16"), m, NS[(m + ksp) % len(NS)], k, **o)
    # 4 + rest: two streaming passes; the second pass's gate, residual and modulate pointers advance by four rows
    for m in (5, 6, 7, 8):
        o = [dict(pro="rms", mod=True, act="swiglu", gate="row", res="out"), dict(act="swiglu", gate="row", res="inplace")][m % 2]
        lo, hi = stream_decide(4, 37, 520, 1, "bf16", {}), stream_decide(m - 4, 37, 520, 1, "bf16", {})
        add(f"split_m{m}_dual_k520_{tag(o)}", f"{lo} + {hi}", m, 37, 520, **o)
        o = [dict(pro="rms", mod=True, gate="row", res="inplace"), dict(bias=True, gate="row", res="out")][m % 2]
        lo, hi = stream_decide(4, 21, 8712, 0, "bf16", {}), stream_decide(m - 4, 21, 8712, 0, "bf16", {})
        add(f"split_m{m}_k8712_{tag(o)}", f"{lo} + {hi}", m, 21, 8712, **o)
    # the persistent loop: three blocks, three or more rounds, a ragged last round - per kernel form
    for wq, dual, k in itertools.product(WQS, (0, 1), (1024, 3072 + 448)):
        n, hooks = (57 if k == 1024 else 13) * (2 if wq == "nf4" else 1) + (0 if wq != "nf4" else -1), {"gemv_blocks": 3}
        o = ops(dual, k + dual)
        add(f"st_pers3_{wq}_d{dual}_k{k}_{tag(o)}", stream_decide(2, n, k, dual, wq, hooks), 2, n, k, wq=wq, hooks=hooks, **o)
    for k in (1024, 2568):
        add(f"st_pers3_m8_k{k}", stream_decide(7, 29, k, 0, "bf16", {}), 7, 29, k, pro="rms", bias=True, hooks={"gemv_blocks": 3})
    # gemv_opt 0 and 15 beside the default 13 (prologue and epilogue-operand load paths), gemv_waves 3 and 8 (block shape)
    for opt, (m, dual, k), pro in itertools.product((0, 15), ((1, 0, 1032), (2, 1, 1032), (4, 0, 3080), (2, 1, 3080), (7, 0, 1024)), ("rms", "none")):
        o = dict(pro=pro, bias=True, gate="row", res="out", **({"act": "swiglu"} if dual else {}))
        add(f"st_opt{opt}_m{m}_d{dual}_k{k}_{tag(o)}", stream_decide(m, 37, k, dual, "bf16", {}), m, 37, k, hooks={"gemv_opt": opt}, **o)
    for waves, n, (m, dual) in itertools.product((3, 8), (10, 33), ((2, 0), (2, 1), (3, 1), (6, 0))):
        o = dict(pro="rms", mod=bool(dual), bias=True, **({"act": "swiglu"} if dual else {}))
        k = 1000 if m > 4 else 1544                      # whole rows per wave (gemv_waves shapes the KSPLIT == 1 blocks only)
        add(f"st_waves{waves}_m{m}_d{dual}_n{n}", stream_decide(m, n, k, dual, "bf16", {}), m, n, k, hooks={"gemv_waves": waves}, **o)

    # ---- rows kernel (process-wide scratch on): each of the 22 instantiations, then the edge forms ---------------------------------------
    S = {"gemv_rows_scratch": 1}

    def rows(cid, m, n, k, dual, f8, hooks=None, want=None, **o):
        hooks = {**S, **(hooks or {})}
        o = {**({"act": "swiglu"} if dual else {}), **o}
        atomic_ok = not dual and o.get("pro", "none") == "none" and o.get("act", "none") == "none" and o.get("res") == "inplace"
        inst, ks0, ksplit, atomic = rows_decide(m, n, k, dual, f8, o.get("mod", False), atomic_ok, hooks)
        assert want is None or inst == _rows(*want), (cid, inst, want)
        add(cid, inst, m, n, k, wq="fp8" if f8 else "bf16", frag=bool(f8) or o.pop("frag", False), hooks=hooks, suffix=f" ksplit={ksplit} atomic={atomic}",
            runs=2 if ksplit == 1 or atomic else 3, **o)
        return ks0, ksplit

    B1 = {"gemv_rows_blocks": 1}
    rows("rows_w4", 3, 48, 1024 - 32, 0, 0, want=(0, 8, 4, 0, 0), pro="rms", bias=True)
    rows("rows_w6", 8, 32, 1536, 0, 0, want=(0, 8, 6, 0, 0), pro="rms", mod=True, gate="row", res="inplace", frag=True)
    rows("rows_w8", 5, 32, 2048 - 32, 0, 0, want=(0, 8, 8, 0, 0), bias=True, act="gelu", gate="chan", res="out")
    rows("rows_d_w4", 4, 32, 1024, 1, 0, want=(1, 8, 4, 0, 0), pro="rms", mod=True, frag=True)
    rows("rows_d_w6", 6, 32, 1536 - 32, 1, 0, want=(1, 8, 6, 0, 0), pro="rms_now", gate="row", res="out")
    rows("rows_d_w8", 7, 32, 2048, 1, 0, want=(1, 8, 8, 0, 0), pro="rms")
    rows("rows_d_p4_7groups", 8, 112, 512 + 32, 1, 0, {"gemv_rows_pers": 3}, want=(1, 8, 4, 1, 0), pro="rms", mod=True, frag=True)
    rows("rows_d_p6_7groups_ragged", 3, 100, 1536, 1, 0, {"gemv_rows_pers": 3}, want=(1, 8, 6, 1, 0), pro="rms", gate="chan", res="out")
    rows("rows_s3", 4, 32, 2048 + 32, 0, 0, want=(0, 4, 3, 0, 0), pro="rms", bias=True, res="out")
    rows("rows_s6", 8, 32, 72 * 32, 0, 0, {"gemv_rows_blocks": 6}, want=(0, 4, 6, 0, 0), bias=True, act="gelu", frag=True)
    rows("rows_s9", 3, 32, 70 * 32, 0, 0, B1, want=(0, 4, 9, 0, 0), pro="rms_now", gate="row", res="inplace")
    rows("rows_s12", 6, 16, 193 * 32, 0, 0, want=(0, 4, 12, 0, 0), pro="rms", bias=True)
    rows("rows_d_s4", 5, 32, 2048 + 64, 1, 0, want=(1, 8, 4, 0, 0), pro="rms", frag=True)
    rows("rows_d_s6", 8, 32, 80 * 32, 1, 0, B1, want=(1, 8, 6, 0, 0), pro="rms", gate="row", res="out")
    rows("rows_d_s8", 4, 32, 128 * 32, 1, 0, B1, want=(1, 8, 8, 0, 0))
    rows("rows_f8_w2", 3, 32, 1024, 0, 1, want=(0, 8, 2, 0, 1), pro="rms", bias=True)
    rows("rows_f8_w4", 8, 48, 2048 - 64, 0, 1, want=(0, 8, 4, 0, 1), bias=True, act="gelu", gate="row", res="out")
    rows("rows_f8_d_w2", 5, 32, 960, 1, 1, want=(1, 8, 2, 0, 1), pro="rms", mod=True)
    rows("rows_f8_d_w4", 6, 32, 2048, 1, 1, want=(1, 8, 4, 0, 1), pro="rms")
    rows("rows_f8_d_p2_7groups", 8, 112, 576, 1, 1, {"gemv_rows_pers": 3}, want=(1, 8, 2, 1, 1), pro="rms", mod=True)
    rows("rows_f8_d_p4_7groups", 4, 112, 1536, 1, 1, {"gemv_rows_pers": 3}, want=(1, 8, 4, 1, 1), pro="rms_now", gate="chan")
    rows("rows_f8_s2", 3, 32, 33 * 64, 0, 1, want=(0, 4, 2, 0, 1), pro="rms", bias=True)
    rows("rows_f8_s4", 7, 32, 33 * 64, 0, 1, {"gemv_rows_blocks": 6}, want=(0, 4, 4, 0, 1), bias=True, res="out")
    rows("rows_f8_s6", 8, 32, 33 * 64, 0, 1, B1, want=(0, 4, 6, 0, 1), pro="rms_now", act="gelu")
    rows("rows_f8_s8", 5, 16, 129 * 64, 0, 1, want=(0, 4, 8, 0, 1), pro="rms", gate="row", res="out")
    rows("rows_f8_d_s2", 4, 32, 33 * 64, 1, 1, want=(1, 8, 2, 0, 1), pro="rms")
    rows("rows_f8_d_s4", 6, 32, 33 * 64, 1, 1, B1, want=(1, 8, 4, 0, 1), gate="row", res="inplace")
    rows("rows_rowmajor_n37", 5, 37, 1024, 0, 0, pro="rms", bias=True, res="out")              # row-major n, not a multiple of 16
    rows("rows_rowmajor_n37_split", 8, 37, 2048 + 96, 0, 0, bias=True, gate="chan", res="out")
    for dual in (0, 1):                                   # "drop K slices that would start past the end": the first (setting, k) where it fires
        hooks, steps = next((h, s) for h in [{}] + [{"gemv_rows_blocks": b} for b in range(1, 33)] for s in range(65, 400)
                            if (lambda r: r and r[1] != r[2])(rows_decide(4, 32, s * 32, dual, 0, False, False, h)))
        ks0, ksplit = rows(f"rows_d{dual}_dropped_slice_k{steps * 32}", 4 + 2 * dual, 32, steps * 32, dual, 0, hooks, pro="rms", bias=not dual)
        assert ksplit < ks0
    rows("rows_inplace_atomic", 8, 32, 2048 + 32, 0, 0, bias=True, gate="row", res="inplace")   # the K slices add into out
    rows("rows_inplace_ticket", 8, 32, 2048 + 32, 0, 0, {"gemv_rows_atomic": 0}, bias=True, gate="row", res="inplace")
    rows("rows_f8_inplace_atomic", 4, 32, 33 * 64, 0, 1, gate="chan", res="inplace")
    rows("rows_f8_inplace_ticket", 4, 32, 33 * 64, 0, 1, {"gemv_rows_atomic": 0}, gate="chan", res="inplace")

    # ---- LDS-staged kernel: fp32 weights at every M, dual and not, the four (KS, NP) forms; bf16 weights where the streaming kernel declines ----
    for w, m, dual, (ks, np_) in itertools.product(("f32", "bf16"), range(1, 9), (0, 1), ((4, 2), (4, 1), (1, 2), (1, 1))):
        inst = _lds(w, m, dual, ks, np_)
        if not lds_built(m, dual, ks, np_):
            continue
        i = next(count)
        n, k = {(4, 2): (1026, 2056), (4, 1): (NS[i % len(NS)], 2048 + 8 * (i % 3)), (1, 2): (8193, 24), (1, 1): (NS[i % len(NS)], 1032 if m == 8 else 520)}[(ks, np_)]
        o = ops(dual, i, (lambda o: o.get("ldx") != 0 or m <= 4) if m * n > 1 else one_output)
        decl = {}
        if w == "bf16":                                   # x 4 bytes off a 16-byte boundary, or (m > 1) rows off the 16-byte grid
            decl = dict(xoff=True) if (i % 2 == 0 or m == 1 or o.get("ldx") == 0) else dict(ldx="k+2")
        assert inst == lds_decide(w, m, n, k, dual)
        add(f"lds_{w}_m{m}_d{dual}_ks{ks}_np{np_}_n{n}_k{k}_{tag(o)}", inst, m, n, k, wq=w, **decl, **o)
    add("lds_f32_m8_two_chunks_k2056", _lds("f32", 8, 0, 4, 1), 8, 33, 2056, wq="f32", pro="rms", mod=True, gate="row", res="out")   # chunks 1024 + 1024 + 8

    # ---- generic kernel: k % 8 != 0, or a weight pointer off 16 bytes; both weight types -----------------------------------------------
    for i, (w, m, k, woff) in enumerate((("f32", 1, 13, False), ("bf16", 2, 13, False), ("f32", 3, 100, False), ("bf16", 8, 1001, False),
                                         ("f32", 5, 64, True), ("bf16", 4, 520, True), ("bf16", 1, 7, False), ("f32", 8, 515, False))):
        o = ops(i % 2, i, lambda o: o.get("ldx") != 0)
        add(f"gen_{w}_m{m}_k{k}{'_woff' if woff else ''}_{tag(o)}", f"gemv_generic<w={w}>", m, NS[i], k, wq=w, woff=woff, **o)
    assert len({c.id for c in cs}) == len(cs), [c.id for c in cs if [d.id for d in cs].count(c.id) > 1]
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
HOST_IDS = [c.id for c in CASES if not c.on_rows]      # the rows route needs the scratch, which is device memory: asserted on the GPU only
# three fixed shapes whose default routes a leaked vv_tune setting would change (m = 3: gemv_rows_scratch; 13 units: gemv_long_ku; dual: gemv_dual_rw)
HYGIENE = [(3, 33, 13 * 512, 0, _stream(4, 0, 4, 4, 2, "bf16")), (2, 33, 1024, 1, _stream(2, 1, 1, 2, 1, "bf16")), (1, 33, 512, 0, _stream(1, 0, 1, 1, 2, "bf16"))]


def instantiation_table():
    lines = []
    for inst in ALL_INSTANTIATIONS:
        ids = [c.id for c in CASES if inst in c.route.split(" + ")]
        sets = [sorted(set(c.hooks) - {"gemv_rows_scratch"}) for c in CASES if c.route == inst]      # reached under default tuning, or under which setting
        hooks = [] if (not sets or [] in sets) else sets[0]
        text = ", ".join(ids[:2]) + (f", ... ({len(ids)} cases)" if len(ids) > 2 else "") + (f"   [{', '.join(hooks)}]" if hooks else "")
        lines.append(f"  {inst:<52} {text}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------
# operands, the fp64 reference and the fp32 stand-in (CPU)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _weights(n, k, wq, which):
    """(what the device reads, its scales or None, the effective matrix as fp64-exact fp32) of one random [n, k] matrix"""
    from vibevoice_rocm_amd.weights import pack_nf4, quantize_e4m3_pow2, quantize_nf4
    g = torch.Generator().manual_seed(zlib.crc32(repr((n, k, wq, which)).encode()))
    w = torch.randn(n, k, generator=g) / k ** 0.5
    if wq == "f32":
        return w, None, w
    if wq == "bf16":
        return w.bfloat16(), None, w.bfloat16().float()
    if wq == "fp8":
        return quantize_e4m3_pow2(w)
    codes, absmax, eff = quantize_nf4(w.bfloat16())
    packed, scales = pack_nf4(codes, absmax)
    return (codes, packed), scales, eff


@functools.lru_cache(maxsize=None)
def _operands_of(key):
    m, n, k, wq, pro, mod, bias, act, gate, res, bcast, on_rows = key
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    o = {"x": torch.randn(1 if bcast else m, k, generator=g)}
    o["w"], o["wscale"], o["w_eff"] = _weights(n, k, wq, 0)
    if act == "swiglu":
        o["w2"], o["w2scale"], o["w2_eff"] = _weights(n, k, wq, 1)
    if pro == "rms":
        o["norm_w"] = 1 + 0.1 * torch.randn(k, generator=g)
    if mod:
        o["shift"], o["scale"] = 0.2 * torch.randn(m, k, generator=g), 0.2 * torch.randn(m, k, generator=g)
    if bias:
        o["bias"] = 0.1 * torch.randn(n, generator=g)
    if gate == "chan":
        o["gate"] = torch.randn(n, generator=g)
    elif gate == "row":
        o["gate"] = torch.randn(m, n, generator=g)
    if res:
        o["res"] = torch.randn(m, n, generator=g)
    return {name: t for name, t in o.items() if t is not None}


def operands(case):
    return _operands_of(case.data_key)


def hi_lo(x):
    """the rows kernel's matrix-core operand pair of an activation: bf16(x) + bf16(x - bf16(x)), as fp64"""
    hi = bf16_round64(x)
    return hi + bf16_round64(x - hi)


def ref_fp64(case, o):
    x = _prologue(o["x"].expand(case.m, case.k), o, case.pro, torch.float64)
    if case.on_rows:
        x = hi_lo(x)
    y = x @ o["w_eff"].double().t()
    y2 = x @ o["w2_eff"].double().t() if "w2_eff" in o else None
    return _epilogue(y, y2, o, case.act, torch.float64)


def figures(got, ref):
    """(global rel RMS, worst row rel RMS, its row, worst element |got - ref| / rms(ref), its index)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = got - ref
    rms = math.sqrt(float(np.mean(ref ** 2))) + 1e-300
    rows = np.sqrt((e ** 2).sum(1) / ((ref ** 2).sum(1) + 1e-300))
    ei = np.unravel_index(np.argmax(np.abs(e)), e.shape)
    return math.sqrt(float(np.mean(e ** 2))) / rms, float(rows.max()), int(np.argmax(rows)), float(np.abs(e).max()) / rms, (int(ei[0]), int(ei[1]))


@functools.lru_cache(maxsize=None)
def _expect_of(key, m, k, pro, act, on_rows):
    """(fp64 reference, floor (global, row, element) of the fp32 stand-in, cost of one dropped 8-column K chunk) for one set of operands"""
    o = _operands_of(key)
    case = Case("", "gemv_rows" if on_rows else "", m, o["w_eff"].shape[0], k, pro=pro, act=act)
    ref = ref_fp64(case, o)
    xh = _prologue(o["x"].expand(m, k), o, pro, torch.float32)
    if on_rows:
        hi = xh.bfloat16().float()
        xh = hi + (xh - hi).bfloat16().float()           # exact in fp32: hi and lo share at most 16 significant bits

    k8 = k - k % 8                                        # the generic kernel's odd tail: one more partial product

    def chunks(w):      # fp32 partial products of the 8-column chunks, and their running sum in order
        n = w.shape[0]
        P = torch.bmm(xh[:, :k8].reshape(m, k // 8, 8).transpose(0, 1), w.reshape(n, k // 8, 8).permute(1, 2, 0))
        return P, torch.cumsum(P, 0)[-1]

    def finish(y, y2):
        return _epilogue(y, y2, o, act, torch.float32).double()

    tail = (lambda w: xh[:, k8:] @ w[:, k8:].t()) if k % 8 else (lambda w: 0.0)
    P, acc = chunks(o["w_eff"][:, :k8].contiguous()) if k8 else (None, 0.0)
    acc = acc + tail(o["w_eff"])
    acc2 = None
    if "w2_eff" in o:
        P2, acc2 = chunks(o["w2_eff"][:, :k8].contiguous()) if k8 else (None, 0.0)
        acc2 = acc2 + tail(o["w2_eff"])
    stand = finish(acc, acc2)
    g, r, _, e, _ = figures(stand, ref)
    rms = math.sqrt(float((ref ** 2).mean()))
    drop = math.inf
    if k8:      # every chunk dropped from every element in turn: the rms of what that costs the element (sqrt(8 / K) of the product's rms, through the epilogue)
        d = _epilogue(acc[None] - P, acc2[None] - P2 if acc2 is not None else None, o, act, torch.float32).double() - stand      # SwiGLU: the chunk leaves both products
        drop = math.sqrt(float((d ** 2).mean())) / rms
    return ref, (g, r, e), drop


def expect(case):
    return _expect_of(case.data_key, case.m, case.k, case.pro, case.act, case.on_rows)


# ---------------------------------------------------------------------------------------------------------------
# CPU-only guards
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CASE_IDS)
def test_bars_sit_between_floor_and_dropped_chunk(cid):
    """Both conditions on the class bar, for every case of the file (CPU only): at least 8 x the fp32 stand-in's own error against the fp64
    reference (global, worst row, worst element), at most a tenth of what one dropped 8-column K chunk costs an element it is dropped from."""
    case = CASES[CASE_IDS.index(cid)]
    _, floor, drop = expect(case)
    bar = BAR[case.klass]
    print(f"{cid}: class {case.klass} bar {bar:.1e}  floor global {floor[0]:.2e} row {floor[1]:.2e} element {floor[2]:.2e}  dropped chunk {drop:.2e}")
    assert bar >= FLOOR_HEADROOM * max(floor), (cid, bar, floor)
    assert bar <= drop / DROP_MARGIN, (cid, bar, drop)


def test_docstring_table_is_current():
    """the instantiation -> case table of the docstring is the one the parametrisation generates, and the instantiations the cases reach are
    exactly the compiled ones: 246 streaming, 22 rows, 108 LDS-staged, 2 generic"""
    assert instantiation_table() in __doc__
    reached = {r for c in CASES for r in c.route.split(" + ")}
    assert reached == set(ALL_INSTANTIATIONS), sorted(reached ^ set(ALL_INSTANTIATIONS))
    assert len(set(ALL_INSTANTIATIONS)) == len(ALL_INSTANTIATIONS) == 378
    assert [sum(i.startswith(p) for i in ALL_INSTANTIATIONS) for p in ("gemv_stream<", "gemv_rows<", "gemv_lds<", "gemv_generic<")] == [246, 22, 108, 2]


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """What is compiled is what can be launched: the gfx950 code objects of the three units hold one kernel per entry of ALL_INSTANTIATIONS and no
    other instantiation of the four templates (CPU only: reads the symbol tables of the object files build() left).  The device side is read
    because the host side proves nothing: launch stubs behind a dead branch vanish while their kernels are still generated.  gemv_rows_kernel's
    weight format 2 (MXFP4) is the other list's: ALL_ROWS_MX of tests/test_host_rowbatch_mxfp4.py, held to exactly that set there; so is
    gemv_stream_kernel's weight format 3 (MXFP4): ALL_MX of tests/test_hip_mxfp4.py."""
    names = {"gemv_stream_kernel": lambda m, dual, ksplit, ku, rw, wq: _stream(m, dual, ksplit, ku, rw, WQS[wq]),
             "gemv_rows_kernel": _rows, "gemv_kernel": _lds, "gemv_generic_kernel": lambda w: f"gemv_generic<w={w}>"}
    got = set()
    for unit in ("vv_gemv_stream.hip", "vv_gemv_rows.hip", "vv_kernels.hip"):
        got |= instantiations_of([(k, args) for k, args in built_kernels(unit, tmp_path) if (k, args[-1]) not in (("gemv_rows_kernel", "2"), ("gemv_stream_kernel", "3"))], names)
    assert got == set(ALL_INSTANTIATIONS), sorted(got ^ set(ALL_INSTANTIATIONS))


def test_reference_agrees_with_ref_linear_of_the_parity_suite():
    """Guards the reference (CPU only): the same function as _ref_linear of test_hip_parity.py for an RMSNorm + modulate + GELU + gate + residual
    call and a SwiGLU one; the rows kernel's hi + lo pair moves it by no more than 2^-17."""
    from test_hip_parity import _ref_linear
    a = Case("g1", "", 3, 40, 64, pro="rms", mod=True, bias=True, act="gelu", gate="row", res="out")
    o = operands(a)
    want = _ref_linear(o["x"], o["w_eff"], None, o["bias"], 1, o["norm_w"], EPS, o["shift"], o["scale"], 1, o["gate"], o["res"])
    assert rel_rms(ref_fp64(a, o).numpy(), want.numpy(), "fp64 reference vs _ref_linear (CPU)") < 1e-12
    b = Case("g2", "gemv_rows", 3, 40, 64, pro="rms", act="swiglu")
    o = operands(b)
    want = _ref_linear(o["x"], o["w_eff"], o["w2_eff"], None, 1, o["norm_w"], EPS, None, None, 2, None, None)
    e = rel_rms(ref_fp64(b, o).numpy(), want.numpy(), "fp64 reference (hi + lo activations) vs _ref_linear (CPU)")
    assert 0 < e < 2.0 ** -16, e


# ---------------------------------------------------------------------------------------------------------------
# the call: layout with NaN gaps and guards, route assertion, launch
# ---------------------------------------------------------------------------------------------------------------
class _tuned:
    """sets the case's vv_tune keys and puts every one back at its default on the way out, whatever happened in between"""

    def __init__(self, hooks):
        self.hooks = hooks

    def __enter__(self):
        L, l = _lib()[:2]
        try:
            for key, v in self.hooks.items():
                L.check(l.vv_tune(key.encode(), v), f"vv_tune {key}")
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        L, l = _lib()[:2]
        for key in self.hooks:
            L.check(l.vv_tune(key.encode(), TUNE_DEFAULTS[key]), f"vv_tune {key}")


def _offset(t, elems):
    """t behind `elems` NaN (or zero, for integer types) elements in one flat allocation: its address is elems elements past the allocation's"""
    flat = torch.full((elems + t.numel(),), NAN if t.is_floating_point() else 0, dtype=t.dtype)
    flat[elems:] = t.reshape(-1)
    return flat


def layout(case, o):
    """The host image of every array the call reads, NaN in every gap, and the strides / element offsets: {name: tensor}, {field: value}"""
    from vibevoice_rocm_amd.weights import DeviceWeights
    m, n, k = case.m, case.n, case.k
    buf, ld = {}, {"x_off": 1 if case.xoff else 0, "w_off": 1 if case.woff else 0}
    if case.ldx == 0:
        x, ld["ldx"] = o["x"].reshape(-1).clone(), 0
    else:
        ld["ldx"] = k + 2 if case.ldx == "k+2" else k + 8
        x = _gapped(o["x"], ld["ldx"]).reshape(-1)
    buf["x"] = _offset(x, ld["x_off"])
    for name in ("w", "w2"):
        if name not in o:
            continue
        w = o[name]
        if case.wq == "nf4":
            w = w[1]
        elif case.frag:
            w = DeviceWeights.frag_major_fp8(w) if case.wq == "fp8" else DeviceWeights.frag_major(w)
            assert w is not None
        buf[name] = _offset(w.contiguous(), ld["w_off"])
        if name + "scale" in o:
            buf[name + "scale"] = o[name + "scale"]
    for name in ("norm_w", "bias"):
        if name in o:
            buf[name] = o[name]
    if case.mod:
        ld["ld_mod"] = 3 * k
        mod = torch.full((m, 3 * k), NAN)
        mod[:, :k], mod[:, k: 2 * k] = o["shift"], o["scale"]
        buf["mod"] = mod
    ld["gate_ld"] = 3 * n if case.gate == "row" else 0
    if case.gate == "chan":
        buf["gate"] = o["gate"]
    elif case.gate == "row":
        buf["gate"] = _gapped(o["gate"], 3 * n, 2 * n)
    ld["ldo"] = n + 3 if case.id.startswith("gen_") else n + 4
    ld["ldres"] = ld["ldo"] if case.res == "inplace" else n + 8
    out = torch.full(((m + 2) * ld["ldo"],), NAN)
    if case.res == "inplace":
        out.view(m + 2, ld["ldo"])[:m, :n] = o["res"]
    elif case.res:
        buf["res"] = _gapped(o["res"], ld["ldres"])
    buf["out"] = out
    return buf, ld


def fill_args(case, ld, ptr):
    """vv_lin_args of the case; ptr: {name: address of the array layout() describes}"""
    L, _ = _lib()[:2]
    m, n, k = case.m, case.n, case.k
    wsz = {"f32": 4, "bf16": 2, "fp8": 1, "nf4": 1}[case.wq]
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.eps = ptr["x"] + 4 * ld["x_off"], ld["ldx"], m, n, k, EPS
    a.wdt = {"f32": L.VV_F32, "bf16": L.VV_BF16, "fp8": L.VV_FP8, "nf4": L.VV_NF4}[case.wq]
    a.w = ptr["w"] + wsz * ld["w_off"]
    a.flags = L.LIN_W_FRAG if case.frag else 0
    a.pro = {"none": L.PRO_NONE, "rms": L.PRO_RMSNORM, "rms_now": L.PRO_RMSNORM, "silu": L.PRO_SILU}[case.pro]
    a.act = {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "swiglu": L.ACT_SWIGLU}[case.act]
    if case.pro == "rms":
        a.norm_w = ptr["norm_w"]
    if case.mod:
        a.mod_shift, a.mod_scale, a.ld_mod = ptr["mod"], ptr["mod"] + 4 * k, ld["ld_mod"]
    if case.dual:
        a.w2 = ptr["w2"] + wsz * ld["w_off"]
    if case.wq in ("fp8", "nf4"):
        a.wscale = ptr["wscale"]
        if case.dual:
            a.w2scale = ptr["w2scale"]
    if case.bias:
        a.bias = ptr["bias"]
    if case.gate:
        a.gate, a.gate_ld = ptr["gate"] + (4 * 2 * n if case.gate == "row" else 0), ld["gate_ld"]
    a.out, a.ldo = ptr["out"], ld["ldo"]
    if case.res == "inplace":
        a.res, a.ldres = a.out, ld["ldo"]
    elif case.res:
        a.res, a.ldres = ptr["res"], ld["ldres"]
    return a


def route_of(a):
    L, l = _lib()[:2]
    name = C.create_string_buffer(192)
    L.check(l.vv_linear_route(C.byref(a), name, 192), "vv_linear_route")
    return name.value.decode()


_FAKE2 = {**_FAKE, "wscale": 0x0d000000, "w2scale": 0x0e000000}


def _plain_route(m, n, k, dual):
    L, _ = _lib()[:2]
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo = _FAKE["x"], k, m, n, k, L.VV_BF16, _FAKE["w"], _FAKE["out"], n
    if dual:
        a.w2, a.act = _FAKE["w2"], L.ACT_SWIGLU
    return route_of(a)


def _hygiene():
    for m, n, k, dual, want in HYGIENE:
        got = _plain_route(m, n, k, dual)
        assert got == want, f"a vv_tune setting leaked: m={m} n={n} k={k} dual={dual} reports {got}, default {want}"


@pytest.mark.parametrize("cid", HOST_IDS)
def test_route_of_every_case_on_the_host(cid):
    """The route query needs no device: every case's arguments (stand-in addresses, aligned as the case says; nothing is dereferenced) report
    the kernel the case is named for, here on the CPU too, and the tune state is back at its defaults afterwards."""
    case = CASES[CASE_IDS.index(cid)]
    _, ld = layout(case, operands(case))
    with _tuned(case.hooks):
        got = route_of(fill_args(case, ld, _FAKE2))
    assert got == case.name, (cid, got, case.name)
    _hygiene()


def test_hot_kernels_by_name_at_their_table_shapes():
    """CPU only: each hot table entry reports gemv_hot<i> / conv_hot_gemv<i> at its own shape and operand set, and the streaming template with the
    entry switched off (vv_tune "gemv_hot" / "conv_hot", restored in the finally)."""
    L, l = _lib()[:2]

    def args(m, n, k, dual, pro, mod, bias, gate_ld, res, flags):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo, a.eps, a.flags = _FAKE["x"], k, m, n, k, L.VV_BF16, _FAKE["w"], _FAKE["out"], n, EPS, flags
        a.pro = pro
        if pro == L.PRO_RMSNORM:
            a.norm_w = _FAKE["norm_w"]
        if mod:
            a.mod_shift, a.mod_scale, a.ld_mod = _FAKE["shift"], _FAKE["scale"], 3 * k
        if dual:
            a.w2, a.act = _FAKE["w2"], L.ACT_SWIGLU
        if bias:
            a.bias = _FAKE["bias"]
        if gate_ld is not None:
            a.gate, a.gate_ld = _FAKE["gate"], gate_ld
        if res:
            a.res, a.ldres = _FAKE["res"], n
        return a

    R, N, W = L.PRO_RMSNORM, L.PRO_NONE, L.LIN_W_REUSED
    hot = [(2, 4608, 1536, 1, R, 1, 0, None, 0, W), (2, 1536, 4608, 0, N, 0, 0, 1536, 1, W), (2, 8960, 1536, 1, R, 0, 0, None, 0, 0),
           (2, 1536, 8960, 0, N, 0, 0, None, 1, 0), (2, 2048, 1536, 0, R, 0, 1, None, 0, 0), (2, 1536, 1536, 0, N, 0, 0, None, 1, 0)]
    conv = {0: (1, 2048, 8192, 0, N, 0, 1, 0, 1, 0), 2: (1, 8192, 4096, 0, N, 0, 1, None, 0, 0), 3: (1, 2048, 16384, 0, N, 0, 1, None, 0, 0)}
    try:
        for i, spec in enumerate(hot):
            assert route_of(args(*spec)) == f"gemv_hot<{i}>"
        for i, spec in conv.items():
            assert route_of(args(*spec)) == f"conv_hot_gemv<{i}>"
        L.check(l.vv_tune(b"gemv_hot", 0), "vv_tune")
        L.check(l.vv_tune(b"conv_hot", 0), "vv_tune")
        for spec in hot + list(conv.values()):
            assert route_of(args(*spec)) == stream_decide(spec[0], spec[1], spec[2], spec[3], "bf16", {})
    finally:
        L.check(l.vv_tune(b"gemv_hot", -1), "vv_tune")
        L.check(l.vv_tune(b"conv_hot", -1), "vv_tune")
    assert route_of(args(*hot[0])) == "gemv_hot<0>"


def test_refused_calls_are_refused_by_the_route_query_too():
    """CPU only: what vv_linear refuses for this family, vv_linear_route refuses with vv_linear's own error text - both take it from the one
    decision (gemv_decide); the stand-in addresses are never handed to vv_linear."""
    L, l = _lib()[:2]
    name = C.create_string_buffer(192)

    def args(m, n, k, wdt, **kw):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo, a.wscale = _FAKE["x"], k, m, n, k, wdt, _FAKE["w"], _FAKE["out"], n, _FAKE2["wscale"]
        for f, v in kw.items():
            setattr(a, f, v)
        return a

    for a, code, text in ((args(3, 32, 1024, L.VV_FP8), -3, "fp8 weights need m <= 2"),                       # fp8 at m = 3 without VV_LIN_W_FRAG
                          (args(3, 32, 1024, L.VV_FP8, flags=L.LIN_W_FRAG), -3, "not covered by the 3..8-row"),   # ... and with it, the scratch off
                          (args(2, 32, 1024, L.VV_NF4, w=_FAKE["w"] + 8), -3, "NF4 weights need"),
                          (args(4, 32, 1024, L.VV_BF16, flags=L.LIN_W_FRAG), -3, "read by the 3..8-row matrix-core GEMV only"),
                          (args(2, 32, 1024, 7), -1, "bad wdt")):
        rc = l.vv_linear_route(C.byref(a), name, 192)
        assert rc == code and text in l.vv_last_error().decode(), (rc, l.vv_last_error())


_MEASURED = {}      # class -> [global, row, element] maxima of this session, written by _report


def run_case(case):
    """Lay the case out, assert its route, launch it `runs` times into separate outputs; returns out[m, n] as fp64"""
    L, l = _lib()[:2]
    o = operands(case)
    buf, ld = layout(case, o)
    m, n, ldo = case.m, case.n, ld["ldo"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda() for _ in range(case.runs)]
    with _tuned(case.hooks):
        for out in outs:
            a = fill_args(case, ld, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
            got_route = route_of(a)
            assert got_route == case.name, (case.id, got_route, case.name)
            L.check(l.vv_linear(C.byref(a), None), "vv_linear")
        torch.cuda.synchronize()
    hs = [t.cpu() for t in outs]
    for name, t in dev.items():
        assert _same_bits(t.cpu(), buf[name]), f"{case.id}: input {name} was written"
    inside = torch.zeros(m + 2, ldo, dtype=torch.bool)
    inside[:m, :n] = True
    for i, h in enumerate(hs):
        grid = h.view(m + 2, ldo)
        assert torch.isfinite(grid[inside]).all(), f"{case.id}: run {i}: {int((~torch.isfinite(grid[inside])).sum())} in-range outputs are not finite"
        assert torch.isnan(grid[~inside]).all(), f"{case.id}: run {i}: a gap or guard element of out was written"
    if case.name.endswith("atomic=1"):                   # fp32 atomics reorder the K slices' sum: every run is held to the bar instead
        return [h.view(m + 2, ldo)[:m, :n].double() for h in hs]
    for i, h in enumerate(hs[1:]):
        assert _same_bits(hs[0], h), f"{case.id}: run {i + 1} of the same call differs from run 0"
    return [hs[0].view(m + 2, ldo)[:m, :n].double()]


pytest_gpu = pytest.mark.gpu


@pytest_gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gemv_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    ref, floor, drop = expect(case)
    bar = BAR[case.klass]
    for got in run_case(case):
        g, r, ri, e, ei = figures(got.numpy(), ref.numpy())
        rel_rms(got.numpy(), ref.numpy(), f"{cid} [{case.name}] global")
        print(f"{cid}: {case.name} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst row {r:.3e} (row {ri})  worst element {e:.3e} at {ei}  "
              f"[floor {max(floor):.2e}, dropped chunk {drop:.2e}]")
        mx = _MEASURED.setdefault(case.klass, [0.0, 0.0, 0.0])
        for i, v in enumerate((g, r, e)):
            mx[i] = max(mx[i], v)
        assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
        assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"
        assert e < bar, f"{cid}: element {ei} is {e:.3e} of the reference's rms from it, >= {bar:.1e}"


@pytest_gpu
def test_zz_tune_state_is_back_at_its_defaults():
    """Hook hygiene: three fixed shapes report their default routes, so a vv_tune setting leaked by any test above - gemv_rows_scratch among
    them, which would send the three-row shape to the matrix cores - fails here."""
    _need_gpu()
    _hygiene()
    _report()


def _report():
    """the session's largest figures per route class, for the docstring and profiles/gemv_parity.txt (written only where VV_GEMV_PARITY_OUT says)"""
    path = os.environ.get("VV_GEMV_PARITY_OUT")
    if not path or not _MEASURED:
        return
    with open(path, "w") as f:
        f.write(f"{torch.cuda.get_device_name(0)}: largest figure against fp64 over each route class's cases (tests/test_hip_gemv.py)\n")
        f.write(f"  {'class':<9} {'cases':>5} {'bar':>8} {'global':>10} {'row':>10} {'element':>10} {'bar / largest':>14}\n")
        for k in BAR:
            if k in _MEASURED:
                g, r, e = _MEASURED[k]
                f.write(f"  {k:<9} {sum(c.klass == k for c in CASES):>5} {BAR[k]:>8.1e} {g:>10.2e} {r:>10.2e} {e:>10.2e} {BAR[k] / max(g, r, e):>14.1f}\n")


if __name__ == "__main__":
    if "--table" in sys.argv:
        print(instantiation_table())
