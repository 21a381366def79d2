// vbs_block_lookup.h -- which block of a ragged batch a sample position lies in.  Blocks of different lengths lie back
// to back; start[0 .. nblocks] are the prefix sums of their lengths (start[0] = 0, start[nblocks] = the batch's
// samples).  Plain C arithmetic on the table alone: K5's ragged block-table mode (k5_verify.hip), the host side of
// api.hip and a host-only compile (tests/test_vbs_ragged_cpu.py) share it, as vbs_schedule.h is shared.
#ifndef FHIP_VBS_BLOCK_LOOKUP_H
#define FHIP_VBS_BLOCK_LOOKUP_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FHIP_LOOKUP_FN static __host__ __device__ inline
#else
#define FHIP_LOOKUP_FN static inline
#endif

// The block b with start[b] <= s < start[b + 1]; nblocks when s lies at or behind the batch's end (s >= start[nblocks]),
// -1 when s < 0.  Every block is at least one sample long, so the b is unique.  A binary search: the uniform mode
// divides where this one halves.
FHIP_LOOKUP_FN int fhip_block_lookup(const long long *start, int nblocks, long long s)
{
    if (s < 0) return -1;
    int lo = 0, hi = nblocks;                     // invariant: start[lo] <= s, and hi == nblocks or s < start[hi]
    if (s >= start[nblocks]) return nblocks;
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (start[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}

#endif
