// libssamd.so: host side of the C ABI declared in include/ssamd.h, include/ssamd_active.h, include/ssamd_graycode.h, include/ssamd_ftp_mapping.h, include/ssamd_structured_light.h and include/ssamd_graycode_stereo.h (gfx950 / ROCm).
// Owns device scratch, chooses launch geometry, launches the HIP kernels.
// There is deliberately no CPU code path for the operators of this library.
// This file is the main translation unit and the map of the host side: the kernel headers, then the host sections (host_*.h), which it
// alone includes, in this order: text of ONE unit (the Lab kernels' __constant__ table and the `extern template` lists exist once).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <list>
#include <map>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ssamd.h"
#include "../../include/ssamd_active.h"
#include "../../include/ssamd_graycode.h"
#include "../../include/ssamd_ftp_mapping.h"
#include "../../include/ssamd_structured_light.h"
#include "../../include/ssamd_graycode_stereo.h"
#include "asw_shared.hip.h"
#include "asw_kernels.hip.h"
#include "asw_pipe_kernel.hip.h"
#include "asw_wave_kernel.hip.h"
#include "asw_wave6_kernel.hip.h"
#include "asw_alt_kernels.hip.h"
#include "asw_prepass_kernels.hip.h"
#include "asw_finalize_kernels.hip.h"
// the phase-shifted and the six-per-lane kernels are instantiated in translation units of their own (asw_pipe_tu.hip, asw_wave6_tu.hip)
namespace ssamd {
#define SSAMD_PIPE_INSTANCE(C, SL, SR, SE) extern template __global__ void asw_aggregate_pipe_kernel<C, SL, SR, SE>(const AswArgs);
#define SSAMD_WAVE6_INSTANCE(C, K) extern template __global__ void asw_aggregate_wave6_kernel<C, K>(const AswWaveArgs);
#include "asw_instances.inc"
#undef SSAMD_PIPE_INSTANCE
#undef SSAMD_WAVE6_INSTANCE
}  // namespace ssamd
#include "gsw_kernels.hip.h"
#include "lab_kernels.hip.h"
#include "asw_exact_kernels.hip.h"
#include "rig_kernels.hip.h"
#include "unwrap_kernels.hip.h"
#include "np_unwrap_kernels.hip.h"
#include "ftp_kernels.hip.h"
#include "ftp_cloud_kernels.hip.h"
#include "ftp_reference_kernels.hip.h"
#include "graycode_kernels.hip.h"
#include "ftp_mapping_kernels.hip.h"
#include "phaseshift_kernels.hip.h"
#include "graycode_stereo_kernels.hip.h"

using namespace ssamd;

// ---- the host side, section by section (each opens at most one anonymous namespace and one extern "C" block)
#include "host_context.h"       // last error, option snapshot (ssamd_options.h) and the planners' headers, DevBuf, profiler, Ctx / get_ctx, ScratchOrder, the host-buffer route
#include "host_geometry.h"      // per-shape geometry caches around the planners, the autotuner's rounds
#include "host_asw.h"           // ASW: tables, kernel variants, AswCall / AswRun and the steps of one call, alternate rows
#include "host_asw_exact.h"     // ASW: the fp64 tie-break pass before and after the aggregation (on the AswRun), its scratch layout, its counters
#include "host_gsw.h"           // GSW: weight table, GswCall, one call
#include "host_matchers.h"      // matcher ABI: HostJob / host_rows / run_strips, every ssamd_asw* and ssamd_gsw* entry point
#include "host_rig.h"           // remap and reproject
#include "host_unwrap.h"        // IIR phase unwrapping
#include "host_np_unwrap.h"     // np.unwrap
#include "host_ftp_phase.h"     // FTP phase
#include "host_ftp_cloud.h"     // FTP cloud
#include "host_ftp_reference.h" // FTP virtual reference image (include/ssamd_active.h)
#include "host_stripe.h"        // FTP central stripe centroids (include/ssamd_active.h)
#include "host_graycode.h"      // Gray-code decode, offsets and cloud (include/ssamd_graycode.h)
#include "host_ftp_mapping.h"   // FTP carrier phase and per-pixel mapping cloud (include/ssamd_ftp_mapping.h)
#include "host_phaseshift.h"    // phase-shift decode and the triangulation of correspondences (include/ssamd_structured_light.h)
#include "host_graycode_stereo.h" // two-camera Gray code: scatter, match, cloud, point pairs (include/ssamd_graycode_stereo.h)
#include "host_library.h"       // version, last error, device count, kernel names, options, counters, autotune switch, geometry queries, profile
#include "host_debug.h"         // verification entry points (ssamd_bgr2lab, ssamd_debug_*) and debug_libm_kernel
