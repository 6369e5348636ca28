// The instantiations of the two aggregation kernel families that are compiled in their own translation units with their own LLVM
// scheduling strategy (build.py; profiles/r05_llvm_sched_strategy_ab.txt): X(template arguments).  ssamd_api.hip declares them
// `extern template`, asw_pipe_tu.hip / asw_wave6_tu.hip define them.  An instantiation missing here is simply compiled in ssamd_api.hip.
#ifdef SSAMD_PIPE_INSTANCE
SSAMD_PIPE_INSTANCE(true, 0, 0, 0)
SSAMD_PIPE_INSTANCE(false, 0, 0, 0)
SSAMD_PIPE_INSTANCE(false, 120, 316, 208)
SSAMD_PIPE_INSTANCE(false, 88, 348, 272)
SSAMD_PIPE_INSTANCE(false, 216, 284, 80)
SSAMD_PIPE_INSTANCE(true, 120, 316, 208)
SSAMD_PIPE_INSTANCE(true, 88, 348, 272)
SSAMD_PIPE_INSTANCE(true, 216, 284, 80)
#endif
#ifdef SSAMD_WAVE6_INSTANCE
SSAMD_WAVE6_INSTANCE(true, 0)
SSAMD_WAVE6_INSTANCE(false, 0)
SSAMD_WAVE6_INSTANCE(false, 2)
SSAMD_WAVE6_INSTANCE(false, 3)
#endif
