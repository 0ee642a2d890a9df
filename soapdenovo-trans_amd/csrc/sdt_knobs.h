/* sdt_knobs.h -- the environment switches of the library and its hosts, in three classes (C and C++):
 *
 *   operational   read in every build:          SDT_TIMING (phase and allocator timings on stderr), SDT_COMM_TIMEOUT_S / SDT_DRAIN_TIMEOUT_S
 *                 sdt_env()                     (deadlines of a multi-rank context's waits), SDT_NO_ARENA (device memory straight from the
 *                                               driver), SDT_PARSE_THREADS (parser threads of the hosts), SDT_SLOW_EXIT (leave through exit():
 *                                               profilers that write their files from an exit handler)
 *   test hooks    honoured only when            shrink a limit or force a path so that SMALL inputs go through it: chunk sizes, pool sizes,
 *                 SDT_TEST_HOOKS=1 is set       receive buffers, workgroup counts, thresholds, the host forms of device phases.  tests/conftest.py
 *                 sdt_test_env()                sets SDT_TEST_HOOKS for the whole suite; a production run ignores every one of them.
 *                                               The two workgroup counts: SDT_SCAN_BLOCKS (lane-per-item kernels: scan_grid) and
 *                                               SDT_WAVE_BLOCKS (wavefront-per-read kernels: wave_blocks of sdt_read_plan.h).
 *   tuning        compiled out unless the       A/B measurement switches (batch sizes, launch sizes, table load, alternative kernels' geometry):
 *                 unit is built -DSDT_TUNING    tools/ab_build.sh builds such variants into gpurun_ab/; the shipped library does not look at them.
 *                 sdt_tuning_env()
 *
 * A production process therefore reads seven variables (the six operational ones and SDT_TEST_HOOKS). */
#ifndef SDT_KNOBS_H
#define SDT_KNOBS_H
#include <stdlib.h>

static inline const char *sdt_env(const char *name) { return getenv(name); }

static inline const char *sdt_test_env(const char *name)
{
	const char *on = getenv("SDT_TEST_HOOKS");
	return on && on[0] == '1' ? getenv(name) : NULL;
}

static inline const char *sdt_tuning_env(const char *name)
{
#ifdef SDT_TUNING
	return getenv(name);
#else
	(void)name;
	return NULL;
#endif
}

/* the size thresholds of the locality pipeline (csrc/sdt_pipeline.hpp: batch, count launch, work item sizes) are tuning switches AND test
 * hooks: tests/test_fullsize_paths.py shrinks them so that inputs of test size take the branches that only a full-size batch reaches.
 * SDT_LAZY_CLEAR=0 is read the same way: sdt_gpu_reset then clears the node table itself instead of leaving the clear to the first
 * launches of the level-1 scatter (sdt_clear_plan.h) -- for A/B runs and tests/test_fused_clear.py */
static inline const char *sdt_size_env(const char *name)
{
	const char *v = sdt_tuning_env(name);
	return v ? v : sdt_test_env(name);
}

static inline int sdt_knob_int(const char *v, int dflt) { return v && *v ? atoi(v) : dflt; }

#endif
