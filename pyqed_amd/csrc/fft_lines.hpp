// fft_lines.hpp — fft_lines (qd_common.hpp) as its two halves, for a caller that transforms many arrays of one shape:
// the plan is a function of (O, L, I) alone (fft_plan.hpp, no device call), the run takes the tables' scratch from the
// open WsScope, builds them and launches.  fft_lines(x, O, L, I, inv, st, &l2) is fft_lines_plan followed by
// fft_lines_run, with *l2 = plan.l2.
#pragma once

#include "fft_plan.hpp"
#include "qd_common.hpp"

namespace qd {

using spog::LinesPlan;
using spog::fft_lines_plan;   // LinesPlan fft_lines_plan(long O, int L, long I)

int fft_lines_run(const LinesPlan& p, c128* x, bool inv, hipStream_t st);

}  // namespace qd
