// lsg_ab.h -- the A/B and test switches.  The shipped library (liblodestar_bls.so) reads no
// environment variable that changes arithmetic or verdict flow: every switch below is a
// compile-time constant there.  The A/B build (liblodestar_bls_ab.so, compiled with -DLSG_AB
// by lodestar_amd/build.py: tests that compare two forms of a stage, bench A/B runs) reads
// them from the environment per call, so one process can compare both forms.
#pragma once
#include <stdlib.h>

// The square roots of sig_decode and h2c_map run their powers with one element per lane
// (k_fp_pow_lanes) from this many power operands per launch on: one per signature, two per
// message (LSG_POW_LANES=0/1, LSG_POW_LANES_MIN=<items> in the A/B build; measured:
// profiles/r17_powlanes_threshold.txt)
#define LSG_POW_LANES_DEFAULT 1
#define LSG_POW_LANES_MIN_DEFAULT 65536

// The bucket pass of the signature MSM (lsg_host.hip run_msm_buckets, lsg_plan.hpp plan_buckets):
// LSG_MSM_FOLD=0 in the A/B build runs it as k_sig_proj + k_seg_reduce<1> on plan_seg's plan instead
// of k_msm_bucket_seg on plan_buckets'; LSG_MSM_IPS=<0..5> forces the latter's lane pairs per bucket
// (log2) for sweeps (profiles/r21_msmfold_ips_sweep.jsonl)
#define LSG_MSM_FOLD_DEFAULT 1
#define LSG_MSM_IPS_DEFAULT (-1)

#ifdef LSG_AB
// integer switch `name`, `dflt` when unset
static inline long lsg_ab_long(const char* name, long dflt) {
  const char* e = getenv(name);
  return e ? atol(e) : dflt;
}
#else
#define lsg_ab_long(name, dflt) ((long)(dflt))
#endif
