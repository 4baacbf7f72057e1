// Kernel-regression metric on the device, train blocks of up to 1024 rows, problems of 9 .. 16 classes: the CLASS-WINDOW form of the
// large solver (include/wdg.h: class windows) as a translation unit of its own.  The source is csrc/kernel_reg_large.hip, compiled
// here with its template argument WIN = true - kr_large_solve_kernel<true> and a copy of the deflation pre-pass - and exporting
// wdg_kernel_regress_large_windows_batched_f32 alone; why it is not a second instantiation beside the first: see there.
//
// replaces: the kernel-regression branch of classifier_based_performance_metric (utils/homophily_metrics.py:283-297,
//           utils/homophily_plot.py:296-310) for graphs of more than 8 classes (utils/util_funcs.py:134,138) at `--sample_max` above
//           533 (homophily_tests.py:54).
#define KL_WINDOWS_UNIT 1
#include "kernel_reg_large.hip"
