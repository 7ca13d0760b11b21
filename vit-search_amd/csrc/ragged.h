// The device's own test of a vr_ragged_plane record (include/vitres_hip.h), shared by the ragged entries of jpeg.hip and
// resample.hip: everything their kernels index a flat buffer with is bounded by what is checked here.
#pragma once
#include "common.h"
#include "../../include/vitres_hip.h"

static_assert(sizeof(vr_ragged_plane) == 32 && sizeof(vr_ragged_plane) % 16 == 0,
              "vr_ragged_plane is 32 bytes: the host marshals the [B] table as 8 int32 per sample");

// C planes of rows x pitch bytes at off, inside a buffer of `bytes`; max_rows / max_pitch: the launch's bounds (they size its grid)
__device__ inline bool rg_plane_ok(const vr_ragged_plane& p, int C, long long bytes, int max_rows, int max_pitch) {
    if (p.off < 0 || (p.off & 15)) return false;
    if (p.pitch < 4 || (p.pitch & 3) || p.pitch > max_pitch) return false;
    if (p.rows < 1 || p.rows > max_rows) return false;
    const long long size = (long long)C * p.rows * p.pitch;             // (C <= 4, rows and pitch below 2^31: no overflow)
    return p.off <= bytes && size <= bytes - p.off;
}
