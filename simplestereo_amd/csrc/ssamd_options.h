// The SSAMD_* experiment / test hooks, each declared ONCE.  Included by host_context.h (a host section of ssamd_api.hip) only, behind the kernel headers.
//   X(name, member of Tuning, type, value when unset, value parsed from the string v (never NULL), forces)
// forces: a condition on the member's value x under which the option forces a kernel form -- such a call neither reads nor writes
// the ASW geometry cache and is not autotuned (asw_geometry_forced).  SSAMD_ASW_STATIC and SSAMD_ASW_EVOL_MAX_MB force although
// the planner never reads them: they change what a trial launch measures.  Struct, assignment, name list and forcing test come from this list.
#pragma once

#define SSAMD_OPTIONS(X) \
    X("SSAMD_ASW_GEOM", asw_geom, std::string, "", v, !x.empty())   /* "XG,DG[,JC[,RX]]" / "XG,DG[,Ty[,Hy]]": forced launch geometry ("" = unset) */ \
    X("SSAMD_GSW_GEOM", gsw_geom, std::string, "", v, false) \
    X("SSAMD_GSW_PLAIN", gsw_plain, int, 0, atoi(v) != 0 ? 1 : 0, false)   /* 1: every GSW call runs gsw_plain_kernel, the reference's loops one thread per pixel (tests: a second standard for the tiled kernel's raw winners) */ \
    X("SSAMD_ASW_PIPE", asw_pipe, int, -1, atoi(v), x >= 0)   /* -1 unset, 0: phase-shifted kernel off, 8 / 16: forced chunk length */ \
    X("SSAMD_ASW_DEPHASE", asw_dephase, int, -1, atoi(v), x >= 0)   /* -1 unset, else the wave order of the phase-shifted kernel */ \
    X("SSAMD_ASW_EVOL", asw_evol, int, 1, atoi(v), x != 1)   /* 0: in-kernel e tiles instead of the TAD volume */ \
    X("SSAMD_ASW_WAVE", asw_wave, int, -1, atoi(v) != 0 ? 1 : 0, x >= 0)   /* -1 unset, 0: small-range wave kernel off (any set value bypasses cache and tuner) */ \
    X("SSAMD_ASW_WAVE_RX", wave_rx, int, 0, atoi(v), x != 0)   /* 0 unset, 8 / 4: forced register tile of the wave kernel */ \
    X("SSAMD_ASW_WAVE_WG", wave_wg, int, 0, std::max(1, std::min(4, atoi(v))), x != 0)   /* 0 unset (one wave per workgroup), 1..4 */ \
    X("SSAMD_ASW_WAVE_UNROLL", wave_unroll, int, 1, atoi(v), false)   /* 0: counted build loop */ \
    X("SSAMD_ASW_WAVE_MERGE", wave_merge, int, 1, atoi(v), x == 0)   /* 0: separate rounds (left and right centres of a strip built one after the other, the round-2 form), else default */ \
    X("SSAMD_ASW_STATIC", asw_static, int, 1, atoi(v), x != 1)   /* 0: the phase-shifted kernel always reads its strides from the geometry (round-2 form); anything else: stride constants where an instantiation has the tile's */ \
    X("SSAMD_ASW_EVOL_MAX_MB", evol_max_mb, int, 0, std::max(0, atoi(v)), x != 0)   /* 0 unset; else a cap of the TAD volume in MiB (tests of the paths taken when memory is short) */ \
    X("SSAMD_ASW_WAVE_RD", wave_rd, int, 0, atoi(v), x != 0)   /* 0: the host decides; 4: never the six-disparities-per-lane form of the wave kernel */ \
    X("SSAMD_ASW_NO_E2", no_e2, bool, false, true, x) \
    X("SSAMD_ASW_XOR_ONLY", xor_only, bool, false, true, x) \
    X("SSAMD_MULTI_ALLOW_REPEAT", multi_allow_repeat, bool, false, true, false) \
    X("SSAMD_ALT_QUEUE_CAP", alt_queue_cap, int, 0, std::max(1, atoi(v)), false)   /* 0 unset */ \
    X("SSAMD_AUTOTUNE", autotune_env, int, -2, atoi(v) > 0 ? 1 : (atoi(v) < 0 ? -1 : 0), false)   /* -2 unset */ \
    X("SSAMD_ASW_EVOL_FAIL", evol_fail, int, 0, atoi(v), false)   /* test hook: 1 = the TAD volume's allocation really fails (a hipMalloc no device can serve) */ \
    X("SSAMD_ASW_COST_KEYS", asw_cost_keys, int, 0, atoi(v) != 0 ? 1 : 0, false)   /* test hook: 1 = ssamd_asw_costs returns the 32-bit cost images of asw_cost_key (bit patterns in the float array) instead of the costs; no kernel form changes */ \
    X("SSAMD_ASW_TAIL", asw_tail, int, -1, atoi(v), false)   /* -1: the host decides; 0: never split the last partial round of workgroups into half-width tiles; 1: whenever possible */ \
    X("SSAMD_ASW_PERSIST", asw_persist, int, -1, atoi(v), x > 0)   /* -1: the host decides; 0: the phase-shifted kernel always runs one workgroup per tile; n > 0: persistent form with min(n, resident slots) workgroups */ \
    X("SSAMD_ASW_PREPASS_FUSE", prepass_fuse, int, 1, atoi(v), false)   /* 0: Lab records and TAD volume as two dependent launches (the form of rounds 2-4) */ \
    X("SSAMD_EXACT_TOL", exact_tol, int, 128, std::max(0, atoi(v)), false)   /* fp64 tie-break pass: candidates within this many ulps of the winning cost image are re-evaluated */ \
    X("SSAMD_EXACT_CAP", exact_cap, int, 0, std::max(1, atoi(v)), false)   /* 0 unset: queue capacity of the tie-break pass in entries (test hook: a tiny queue overflows) */ \
    X("SSAMD_EXACT_RAWCAP", exact_rawcap, int, 0, std::max(1, atoi(v)), false)   /* 0 unset: capacity of the RAW queue of merging calls (test hook) */ \
    X("SSAMD_UNWRAP_ROWS", unwrap_rows, int, 0, std::max(0, std::min(UNWRAP_MAX_ROWS, atoi(v))), false)   /* 0 unset: most rows per band of the unwrapping wavefront (64..1024, rounded up to 64) */

struct Tuning {
#define X(NAME, MEMBER, TYPE, UNSET, PARSE, FORCES) TYPE MEMBER = UNSET;
    SSAMD_OPTIONS(X)
#undef X
};

// v == nullptr: back to the unset value.  false: no such option.
bool tuning_assign(Tuning &t, const std::string &name, const char *v)
{
#define X(NAME, MEMBER, TYPE, UNSET, PARSE, FORCES) \
    if (name == NAME) { if (v) t.MEMBER = PARSE; else t.MEMBER = UNSET; return true; }
    SSAMD_OPTIONS(X)
#undef X
    return false;
}

const char *const kTuningNames[] = {
#define X(NAME, MEMBER, TYPE, UNSET, PARSE, FORCES) NAME,
    SSAMD_OPTIONS(X)
#undef X
};

// experiment / test hooks that force a kernel form: such calls neither read nor write the geometry cache and are not autotuned
bool asw_geometry_forced(const Tuning &t)
{
#define X(NAME, MEMBER, TYPE, UNSET, PARSE, FORCES) { const TYPE &x = t.MEMBER; (void)x; if (FORCES) return true; }
    SSAMD_OPTIONS(X)
#undef X
    return false;
}
