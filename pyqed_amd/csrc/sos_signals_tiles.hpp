// sos_signals_tiles.hpp — the constants that bound a tile or a loop in sos_signals.hip.  tests/test_sos_signals_gpu.py
// runs sizes C - 1, C, C + 1 on the dimension each of them governs; keep its table in step with this file.
#pragma once

namespace qd {

// threads per workgroup of every kernel in sos_signals.hip; also the y points one workgroup of the inner pass covers,
// the (p, q) table entries one workgroup of the build pass covers and the grid points one workgroup of the TPA kernel
// covers (one per thread)
constexpr int SOS_THREADS = 256;
// inner pass: (zy, W) pairs of one row p staged through LDS per round
constexpr int SOS_QCHUNK = 256;
// outer pass: the output tile is SOS_TILE x SOS_TILE grid points, one per thread
constexpr int SOS_TILE = 16;
// outer pass: poles whose x factors and T rows are staged through LDS per round
constexpr int SOS_PCHUNK = 64;

static_assert(SOS_TILE * SOS_TILE == SOS_THREADS, "one output point per thread");
static_assert(SOS_QCHUNK == SOS_THREADS, "the inner pass stages one (zy, W) pair per thread");
static_assert((SOS_PCHUNK * SOS_TILE) % SOS_THREADS == 0, "the outer pass stages whole rounds of entries");

}  // namespace qd
