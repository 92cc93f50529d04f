// mifc_stencil_limits.h -- the launch-size thresholds the stencil launchers share (mifc_vortdiv_plan.h,
// mifc_stencil_rows.hip, mifc_stencil_split.hip).  Part of mifc_kernels.h; a file of its own only so that the
// host-only planner can see them without the HIP runtime header.
#ifndef MIFC_STENCIL_LIMITS_H
#define MIFC_STENCIL_LIMITS_H

namespace mifc {

// A launch of fewer waves than this is latency-bound (the reference's single-field call): shorter bands, or a form without a row loop.
constexpr long kSmallLaunchWaves = 2048;
// When the level-walking forms take over from the row-walking one (measured: profiles/r02/experiments/levelwalk_threshold.txt);
// MIFC_LEVELWALK_MIN_UNITS overrides the units.
constexpr int kLevelWalkMinLevels = 3;
constexpr long kLevelWalkMinUnits = 768;
// From this many workgroups per level on, tested launches leave their counts in StencilParams::partials instead of one atomic each.
constexpr long kPartialCountUnitsPerLevel = 2048;
// Workgroup units are decoded with 32-bit arithmetic (sequence -> level, band, column): a launch beyond this many is declined.
constexpr long kUnitIndexLimit = 0x3fffffffL;

} // namespace mifc

#endif // MIFC_STENCIL_LIMITS_H
