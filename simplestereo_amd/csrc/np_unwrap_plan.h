// Host planner of the numpy-style phase unwrapper (np_unwrap_kernels.hip.h): which kernel form scans a geometry and its launch
// shape.  Pure arithmetic, like asw_plan.h, gsw_plan.h and ftp_plan.h; needs no device.  The kernels take their chunk and tile
// sizes from the constants below, so what ssamd_np_unwrap_plan reports is what runs.
//
// Any C-contiguous n-D array and axis are one geometry [outer][len][inner]: the scan runs along len at stride inner.
//   row form     inner == 1: the scanned axis is contiguous.  One wave (a workgroup of 64 threads) per line, NPU_ROW_CHUNK
//                samples at a time through LDS; the line's last sample and running sum are carried from chunk to chunk.
//   column form  inner > 1: lanes along inner.  A workgroup of 256 threads owns NPU_COL_LANES neighbouring columns of one
//                outer index and goes down len in tiles of NPU_COL_ROWS rows (every thread NPU_COL_PER consecutive rows of one
//                column); each column's last sample and running sum are carried from tile to tile.
// Neither form limits len.  What is refused is what the launch cannot index -- a HIP launch must stay below 2^32 threads
// (gridDim.x * blockDim.x), so at most 2^26 - 1 lines (row form) or 2^24 - 1 workgroups (column form) -- and more elements than
// the host-buffer path stages (2^40, as ssamd_iir_unwrap).
#pragma once
#include <stdint.h>

constexpr int NPU_ROW_THREADS = 64;
constexpr int NPU_ROW_PER = 8;                                       // samples per lane and chunk
constexpr int NPU_ROW_CHUNK = NPU_ROW_THREADS * NPU_ROW_PER;         // 512
constexpr int NPU_COL_THREADS = 256;
constexpr int NPU_COL_LANES = 16;                                    // 128 bytes of a row per workgroup: one cache line
constexpr int NPU_COL_PER = 8;                                       // consecutive rows per thread and tile: 8 + 1 loads in flight
constexpr int NPU_COL_ROWS = NPU_COL_THREADS / NPU_COL_LANES * NPU_COL_PER;      // 128
constexpr int NPU_WALK = 8;                                          // corrections the serial lane reads ahead of its add chain
constexpr long long NPU_MAX_ELEMS = 1ll << 40;
constexpr long long NPU_MAX_LAUNCH_THREADS = (1ll << 32) - 1;        // gridDim.x * blockDim.x of one launch

enum NpuVerdict { NPU_OK = 0, NPU_NEGATIVE, NPU_TOO_MANY_ELEMS, NPU_TOO_MANY_BLOCKS };

struct NpuPlan {
    int form;               // 0 row, 1 column
    int chunk;              // samples (row form) or rows (column form) between two hand-overs of the carried state
    int lanes;              // lanes along the contiguous axis: 64 along the line (row form), NPU_COL_LANES columns (column form)
    int threads;
    long long blocks;       // 0: an empty extent, nothing to launch
    int lds_bytes;          // static LDS of the kernel
    int per_thread;         // samples per thread and chunk
    long long groups;       // column form: lane groups per outer index
};

inline NpuVerdict npu_plan(long long outer, long long len, long long inner, NpuPlan &p)
{
    if (outer < 0 || len < 0 || inner < 0) return NPU_NEGATIVE;
    const bool row = inner <= 1;
    p.form = row ? 0 : 1;
    p.chunk = row ? NPU_ROW_CHUNK : NPU_COL_ROWS;
    p.lanes = row ? NPU_ROW_THREADS : NPU_COL_LANES;
    p.threads = row ? NPU_ROW_THREADS : NPU_COL_THREADS;
    p.per_thread = row ? NPU_ROW_PER : NPU_COL_PER;
    // corrections / running sums of one chunk (+ the read-ahead of the serial lane past its end); column form: + a row of carried samples
    p.lds_bytes = row ? (NPU_ROW_CHUNK + NPU_WALK) * 8 : ((NPU_COL_ROWS + NPU_WALK) * NPU_COL_LANES + NPU_COL_LANES) * 8;
    p.blocks = 0;
    p.groups = 0;
    if (outer == 0 || len == 0 || inner == 0) return NPU_OK;
    if (outer > NPU_MAX_ELEMS || len > NPU_MAX_ELEMS || inner > NPU_MAX_ELEMS) return NPU_TOO_MANY_ELEMS;
    if (outer > NPU_MAX_ELEMS / len || outer * len > NPU_MAX_ELEMS / inner) return NPU_TOO_MANY_ELEMS;
    p.groups = row ? 1 : (inner + NPU_COL_LANES - 1) / NPU_COL_LANES;
    p.blocks = outer * p.groups;                 // <= 2^40: no overflow
    return p.blocks > NPU_MAX_LAUNCH_THREADS / p.threads ? NPU_TOO_MANY_BLOCKS : NPU_OK;
}
