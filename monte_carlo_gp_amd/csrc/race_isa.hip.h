// race_isa.hip.h -- the few gfx950 instructions the race kernels issue directly (inline assembly).
#ifndef MCGP_RACE_ISA_H
#define MCGP_RACE_ISA_H
#include <hip/hip_runtime.h>

namespace mcgp {

// v_min_f64 / v_max_f64 issued directly: through fmin()/fmax() hipcc adds a canonicalising
// v_max_f64 x, x, x per operand (IEEE mode quiets signalling NaNs), tripling the cost.  Times are
// finite and non-negative here, for which the bare instructions are exact.  Plain VALU, interlocked
// by hardware: no wait states needed inside the statement.
__device__ __forceinline__ void minmax_f64(double a, double b, double &lo, double &hi)
{
    asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(a), "v"(b));
    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(a), "v"(b));
}

__device__ __forceinline__ double max_f64(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// max(|a|, b): the magnitude of a through the instruction's source modifier (no extra instruction)
__device__ __forceinline__ double max_abs_f64(double a, double b)
{
    double r;
    asm("v_max_f64 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Compare-exchange on the time alone, the payload word following its time: after it (ca, pa) holds the smaller
// time.  Equal times are left as they are (stable).  One statement so that the two f64 selects sit between the
// compare and the payload selects: the v_cmp -> v_cndmask (VCC) dependency needs two wait states, and the compiler
// left to itself pads them with an s_nop per comparator.
__device__ __forceinline__ void cmpx_time(double &ca, uint32_t &pa, double &cb, uint32_t &pb)
{
    double lo, hi;
    uint32_t p0, p1;
    asm("v_cmp_gt_f64 vcc, %[a], %[b]\n\t"
        "v_min_f64 %[lo], %[a], %[b]\n\t"
        "v_max_f64 %[hi], %[a], %[b]\n\t"
        "v_cndmask_b32 %[p0], %[pa], %[pb], vcc\n\t"
        "v_cndmask_b32 %[p1], %[pb], %[pa], vcc"
        : [lo] "=&v"(lo), [hi] "=&v"(hi), [p0] "=&v"(p0), [p1] "=&v"(p1)
        : [a] "v"(ca), [b] "v"(cb), [pa] "v"(pa), [pb] "v"(pb)
        : "vcc");
    ca = lo; cb = hi; pa = p0; pb = p1;
}

// ---- merged comparators ----
// hipcc pads every inline-asm statement that touches VCC with an s_nop; several comparators per statement
// amortise it (and keep the v_cmp -> v_cndmask spacing without padding).  All are compare-exchanges on the time
// alone with the payload word following its time, exactly cmpx_time.

// two independent comparators (a1, b1) and (a2, b2)
__device__ __forceinline__ void cmpx_time2(double &a1, uint32_t &pa1, double &b1, uint32_t &pb1,
                                           double &a2, uint32_t &pa2, double &b2, uint32_t &pb2)
{
    double lo1, hi1, lo2, hi2;
    uint32_t x1, y1, x2, y2;
    asm(
        "v_cmp_gt_f64 vcc, %[a1], %[b1]\n\t"
        "v_min_f64 %[lo1], %[a1], %[b1]\n\t"
        "v_max_f64 %[hi1], %[a1], %[b1]\n\t"
        "v_cndmask_b32 %[x1], %[pa1], %[pb1], vcc\n\t"
        "v_cndmask_b32 %[y1], %[pb1], %[pa1], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[a2], %[b2]\n\t"
        "v_min_f64 %[lo2], %[a2], %[b2]\n\t"
        "v_max_f64 %[hi2], %[a2], %[b2]\n\t"
        "v_cndmask_b32 %[x2], %[pa2], %[pb2], vcc\n\t"
        "v_cndmask_b32 %[y2], %[pb2], %[pa2], vcc"
        : [lo1] "=&v"(lo1), [hi1] "=&v"(hi1), [x1] "=&v"(x1), [y1] "=&v"(y1), [lo2] "=&v"(lo2), [hi2] "=&v"(hi2),
          [x2] "=&v"(x2), [y2] "=&v"(y2)
        : [a1] "v"(a1), [b1] "v"(b1), [pa1] "v"(pa1), [pb1] "v"(pb1), [a2] "v"(a2), [b2] "v"(b2), [pa2] "v"(pa2),
          [pb2] "v"(pb2)
        : "vcc");
    a1 = lo1; b1 = hi1; pa1 = x1; pb1 = y1;
    a2 = lo2; b2 = hi2; pa2 = x2; pb2 = y2;
}

// forward bubble over 3 consecutive slots: comparators (0,1), (1,2), .. in sequence, the maximum ends in the last
__device__ __forceinline__ void bubble_fwd2(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2)
{
    double lo1, h1, lo2, h2;
    uint32_t q1, r1, q2, r2;
    asm(
        "v_cmp_gt_f64 vcc, %[c0], %[c1]\n\t"
        "v_min_f64 %[lo1], %[c0], %[c1]\n\t"
        "v_max_f64 %[h1], %[c0], %[c1]\n\t"
        "v_cndmask_b32 %[q1], %[p0], %[p1], vcc\n\t"
        "v_cndmask_b32 %[r1], %[p1], %[p0], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[h1], %[c2]\n\t"
        "v_min_f64 %[lo2], %[h1], %[c2]\n\t"
        "v_max_f64 %[h2], %[h1], %[c2]\n\t"
        "v_cndmask_b32 %[q2], %[r1], %[p2], vcc\n\t"
        "v_cndmask_b32 %[r2], %[p2], %[r1], vcc"
        : [lo1] "=&v"(lo1), [h1] "=&v"(h1), [q1] "=&v"(q1), [r1] "=&v"(r1), [lo2] "=&v"(lo2), [h2] "=&v"(h2), [q2] "=&v"(q2), [r2] "=&v"(r2)
        : [c0] "v"(c0), [p0] "v"(p0), [c1] "v"(c1), [p1] "v"(p1), [c2] "v"(c2), [p2] "v"(p2)
        : "vcc");
    c0 = lo1; p0 = q1;
    c1 = lo2; p1 = q2;
    c2 = h2; p2 = r2;
}

// backward bubble over 3 consecutive slots: comparators (1,2), (0,1), .. in sequence, the minimum ends in slot 0
__device__ __forceinline__ void bubble_bwd2(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2)
{
    double l1, hi1, l2, hi2;
    uint32_t q1, r1, q2, r2;
    asm(
        "v_cmp_gt_f64 vcc, %[c1], %[c2]\n\t"
        "v_min_f64 %[l1], %[c1], %[c2]\n\t"
        "v_max_f64 %[hi1], %[c1], %[c2]\n\t"
        "v_cndmask_b32 %[q1], %[p1], %[p2], vcc\n\t"
        "v_cndmask_b32 %[r1], %[p2], %[p1], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[c0], %[l1]\n\t"
        "v_min_f64 %[l2], %[c0], %[l1]\n\t"
        "v_max_f64 %[hi2], %[c0], %[l1]\n\t"
        "v_cndmask_b32 %[q2], %[p0], %[q1], vcc\n\t"
        "v_cndmask_b32 %[r2], %[q1], %[p0], vcc"
        : [l1] "=&v"(l1), [hi1] "=&v"(hi1), [q1] "=&v"(q1), [r1] "=&v"(r1), [l2] "=&v"(l2), [hi2] "=&v"(hi2), [q2] "=&v"(q2), [r2] "=&v"(r2)
        : [c0] "v"(c0), [p0] "v"(p0), [c1] "v"(c1), [p1] "v"(p1), [c2] "v"(c2), [p2] "v"(p2)
        : "vcc");
    c2 = hi1; p2 = r1;
    c1 = hi2; p1 = r2;
    c0 = l2; p0 = q2;
}

// forward bubble over 4 consecutive slots: comparators (0,1), (1,2), .. in sequence, the maximum ends in the last
__device__ __forceinline__ void bubble_fwd3(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3)
{
    double lo1, h1, lo2, h2, lo3, h3;
    uint32_t q1, r1, q2, r2, q3, r3;
    asm(
        "v_cmp_gt_f64 vcc, %[c0], %[c1]\n\t"
        "v_min_f64 %[lo1], %[c0], %[c1]\n\t"
        "v_max_f64 %[h1], %[c0], %[c1]\n\t"
        "v_cndmask_b32 %[q1], %[p0], %[p1], vcc\n\t"
        "v_cndmask_b32 %[r1], %[p1], %[p0], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[h1], %[c2]\n\t"
        "v_min_f64 %[lo2], %[h1], %[c2]\n\t"
        "v_max_f64 %[h2], %[h1], %[c2]\n\t"
        "v_cndmask_b32 %[q2], %[r1], %[p2], vcc\n\t"
        "v_cndmask_b32 %[r2], %[p2], %[r1], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[h2], %[c3]\n\t"
        "v_min_f64 %[lo3], %[h2], %[c3]\n\t"
        "v_max_f64 %[h3], %[h2], %[c3]\n\t"
        "v_cndmask_b32 %[q3], %[r2], %[p3], vcc\n\t"
        "v_cndmask_b32 %[r3], %[p3], %[r2], vcc"
        : [lo1] "=&v"(lo1), [h1] "=&v"(h1), [q1] "=&v"(q1), [r1] "=&v"(r1), [lo2] "=&v"(lo2), [h2] "=&v"(h2), [q2] "=&v"(q2), [r2] "=&v"(r2), [lo3] "=&v"(lo3), [h3] "=&v"(h3), [q3] "=&v"(q3), [r3] "=&v"(r3)
        : [c0] "v"(c0), [p0] "v"(p0), [c1] "v"(c1), [p1] "v"(p1), [c2] "v"(c2), [p2] "v"(p2), [c3] "v"(c3), [p3] "v"(p3)
        : "vcc");
    c0 = lo1; p0 = q1;
    c1 = lo2; p1 = q2;
    c2 = lo3; p2 = q3;
    c3 = h3; p3 = r3;
}

// backward bubble over 4 consecutive slots: comparators (2,3), (1,2), .. in sequence, the minimum ends in slot 0
__device__ __forceinline__ void bubble_bwd3(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3)
{
    double l1, hi1, l2, hi2, l3, hi3;
    uint32_t q1, r1, q2, r2, q3, r3;
    asm(
        "v_cmp_gt_f64 vcc, %[c2], %[c3]\n\t"
        "v_min_f64 %[l1], %[c2], %[c3]\n\t"
        "v_max_f64 %[hi1], %[c2], %[c3]\n\t"
        "v_cndmask_b32 %[q1], %[p2], %[p3], vcc\n\t"
        "v_cndmask_b32 %[r1], %[p3], %[p2], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[c1], %[l1]\n\t"
        "v_min_f64 %[l2], %[c1], %[l1]\n\t"
        "v_max_f64 %[hi2], %[c1], %[l1]\n\t"
        "v_cndmask_b32 %[q2], %[p1], %[q1], vcc\n\t"
        "v_cndmask_b32 %[r2], %[q1], %[p1], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[c0], %[l2]\n\t"
        "v_min_f64 %[l3], %[c0], %[l2]\n\t"
        "v_max_f64 %[hi3], %[c0], %[l2]\n\t"
        "v_cndmask_b32 %[q3], %[p0], %[q2], vcc\n\t"
        "v_cndmask_b32 %[r3], %[q2], %[p0], vcc"
        : [l1] "=&v"(l1), [hi1] "=&v"(hi1), [q1] "=&v"(q1), [r1] "=&v"(r1), [l2] "=&v"(l2), [hi2] "=&v"(hi2), [q2] "=&v"(q2), [r2] "=&v"(r2), [l3] "=&v"(l3), [hi3] "=&v"(hi3), [q3] "=&v"(q3), [r3] "=&v"(r3)
        : [c0] "v"(c0), [p0] "v"(p0), [c1] "v"(c1), [p1] "v"(p1), [c2] "v"(c2), [p2] "v"(p2), [c3] "v"(c3), [p3] "v"(p3)
        : "vcc");
    c3 = hi1; p3 = r1;
    c2 = hi2; p2 = r2;
    c1 = hi3; p1 = r3;
    c0 = l3; p0 = q3;
}

// forward bubble over 5 consecutive slots: comparators (0,1), (1,2), .. in sequence, the maximum ends in the last
__device__ __forceinline__ void bubble_fwd4(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3, double &c4, uint32_t &p4)
{
    double lo1, h1, lo2, h2, lo3, h3, lo4, h4;
    uint32_t q1, r1, q2, r2, q3, r3, q4, r4;
    asm(
        "v_cmp_gt_f64 vcc, %[c0], %[c1]\n\t"
        "v_min_f64 %[lo1], %[c0], %[c1]\n\t"
        "v_max_f64 %[h1], %[c0], %[c1]\n\t"
        "v_cndmask_b32 %[q1], %[p0], %[p1], vcc\n\t"
        "v_cndmask_b32 %[r1], %[p1], %[p0], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[h1], %[c2]\n\t"
        "v_min_f64 %[lo2], %[h1], %[c2]\n\t"
        "v_max_f64 %[h2], %[h1], %[c2]\n\t"
        "v_cndmask_b32 %[q2], %[r1], %[p2], vcc\n\t"
        "v_cndmask_b32 %[r2], %[p2], %[r1], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[h2], %[c3]\n\t"
        "v_min_f64 %[lo3], %[h2], %[c3]\n\t"
        "v_max_f64 %[h3], %[h2], %[c3]\n\t"
        "v_cndmask_b32 %[q3], %[r2], %[p3], vcc\n\t"
        "v_cndmask_b32 %[r3], %[p3], %[r2], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[h3], %[c4]\n\t"
        "v_min_f64 %[lo4], %[h3], %[c4]\n\t"
        "v_max_f64 %[h4], %[h3], %[c4]\n\t"
        "v_cndmask_b32 %[q4], %[r3], %[p4], vcc\n\t"
        "v_cndmask_b32 %[r4], %[p4], %[r3], vcc"
        : [lo1] "=&v"(lo1), [h1] "=&v"(h1), [q1] "=&v"(q1), [r1] "=&v"(r1), [lo2] "=&v"(lo2), [h2] "=&v"(h2), [q2] "=&v"(q2), [r2] "=&v"(r2), [lo3] "=&v"(lo3), [h3] "=&v"(h3), [q3] "=&v"(q3), [r3] "=&v"(r3), [lo4] "=&v"(lo4), [h4] "=&v"(h4), [q4] "=&v"(q4), [r4] "=&v"(r4)
        : [c0] "v"(c0), [p0] "v"(p0), [c1] "v"(c1), [p1] "v"(p1), [c2] "v"(c2), [p2] "v"(p2), [c3] "v"(c3), [p3] "v"(p3), [c4] "v"(c4), [p4] "v"(p4)
        : "vcc");
    c0 = lo1; p0 = q1;
    c1 = lo2; p1 = q2;
    c2 = lo3; p2 = q3;
    c3 = lo4; p3 = q4;
    c4 = h4; p4 = r4;
}

// backward bubble over 5 consecutive slots: comparators (3,4), (2,3), .. in sequence, the minimum ends in slot 0
__device__ __forceinline__ void bubble_bwd4(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3, double &c4, uint32_t &p4)
{
    double l1, hi1, l2, hi2, l3, hi3, l4, hi4;
    uint32_t q1, r1, q2, r2, q3, r3, q4, r4;
    asm(
        "v_cmp_gt_f64 vcc, %[c3], %[c4]\n\t"
        "v_min_f64 %[l1], %[c3], %[c4]\n\t"
        "v_max_f64 %[hi1], %[c3], %[c4]\n\t"
        "v_cndmask_b32 %[q1], %[p3], %[p4], vcc\n\t"
        "v_cndmask_b32 %[r1], %[p4], %[p3], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[c2], %[l1]\n\t"
        "v_min_f64 %[l2], %[c2], %[l1]\n\t"
        "v_max_f64 %[hi2], %[c2], %[l1]\n\t"
        "v_cndmask_b32 %[q2], %[p2], %[q1], vcc\n\t"
        "v_cndmask_b32 %[r2], %[q1], %[p2], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[c1], %[l2]\n\t"
        "v_min_f64 %[l3], %[c1], %[l2]\n\t"
        "v_max_f64 %[hi3], %[c1], %[l2]\n\t"
        "v_cndmask_b32 %[q3], %[p1], %[q2], vcc\n\t"
        "v_cndmask_b32 %[r3], %[q2], %[p1], vcc\n\t"
        "v_cmp_gt_f64 vcc, %[c0], %[l3]\n\t"
        "v_min_f64 %[l4], %[c0], %[l3]\n\t"
        "v_max_f64 %[hi4], %[c0], %[l3]\n\t"
        "v_cndmask_b32 %[q4], %[p0], %[q3], vcc\n\t"
        "v_cndmask_b32 %[r4], %[q3], %[p0], vcc"
        : [l1] "=&v"(l1), [hi1] "=&v"(hi1), [q1] "=&v"(q1), [r1] "=&v"(r1), [l2] "=&v"(l2), [hi2] "=&v"(hi2), [q2] "=&v"(q2), [r2] "=&v"(r2), [l3] "=&v"(l3), [hi3] "=&v"(hi3), [q3] "=&v"(q3), [r3] "=&v"(r3), [l4] "=&v"(l4), [hi4] "=&v"(hi4), [q4] "=&v"(q4), [r4] "=&v"(r4)
        : [c0] "v"(c0), [p0] "v"(p0), [c1] "v"(c1), [p1] "v"(p1), [c2] "v"(c2), [p2] "v"(p2), [c3] "v"(c3), [p3] "v"(p3), [c4] "v"(c4), [p4] "v"(p4)
        : "vcc");
    c4 = hi1; p4 = r1;
    c3 = hi2; p3 = r2;
    c2 = hi3; p2 = r3;
    c1 = hi4; p1 = r4;
    c0 = l4; p0 = q4;
}

// ---- selects through VCC ----
// A select whose mask sits in an SGPR pair is VOP3-encoded (v_cndmask_b32_e64) and occupies the SIMD for ~4.2 cycles; the
// VOP2 form, which reads its mask from VCC, for ~2.3 (tools/valu_peak.hip).  Where one compare feeds several selects the
// block is written out: the compare into VCC, the selects right behind.  gfx950 needs two wait states between a VALU write
// of VCC and a VALU read of it and does not interlock them: at least two independent instructions sit in between.

// One adjacent pair of an overtake pass (reference :516-524, pace deltas x 2^31): the pair is a candidate iff dl > od
// (NaN -- a retired car -- is not); thr = the draw-word threshold min(ceil(dl), 2^31) of a candidate, 0 otherwise; `next` =
// `row` advanced by `stride` for a candidate, so that the W-plane address of a pair's draw word is a running sum over the
// pairs before it instead of a popcount.  (STRIDE is an assembly-time literal: a register holding it would be one more
// value alive across the whole pass.)
// CEIL = false (the reference-width build): thr = min(floor(dl), 2^31) -- the conversion truncates by itself.
template <uint32_t STRIDE, bool CEIL = true>
__device__ __forceinline__ void ovt_threshold(double dl, double od, uint32_t row, uint32_t &thr, uint32_t &next)
{
    if constexpr (CEIL) {
        double t;
        asm("v_cmp_lt_f64 vcc, %[od], %[dl]\n\t"
            "v_ceil_f64 %[t], %[dl]\n\t"
            "v_cvt_u32_f64 %[thr], %[t]\n\t"
            "v_min_u32 %[thr], 0x80000000, %[thr]\n\t"
            "v_add_u32 %[next], %[stride], %[row]\n\t"
            "v_cndmask_b32 %[thr], 0, %[thr], vcc\n\t"
            "v_cndmask_b32 %[next], %[row], %[next], vcc"
            : [t] "=&v"(t), [thr] "=&v"(thr), [next] "=&v"(next)
            : [dl] "v"(dl), [od] "s"(od), [row] "v"(row), [stride] "n"(STRIDE)
            : "vcc");
    } else {
        asm("v_cmp_lt_f64 vcc, %[od], %[dl]\n\t"
            "v_cvt_u32_f64 %[thr], %[dl]\n\t"
            "v_add_u32 %[next], %[stride], %[row]\n\t"
            "v_min_u32 %[thr], 0x80000000, %[thr]\n\t"
            "v_cndmask_b32 %[next], %[row], %[next], vcc\n\t"
            "v_cndmask_b32 %[thr], 0, %[thr], vcc"
            : [thr] "=&v"(thr), [next] "=&v"(next)
            : [dl] "v"(dl), [od] "s"(od), [row] "v"(row), [stride] "n"(STRIDE)
            : "vcc");
    }
}

// The same pair under EXEC, with the fetch of its draw word inside the statement.  ovt_threshold computes a threshold and
// an advanced row for every lane and then drops both, by two selects, for the pairs that are no candidates -- all but 3
// or 4 of a lane's 19.  Here, under the entry mask:  thr = 0;  ow = the word at W-plane address `row` (the LDS block's
// W plane starts at OW, an immediate of the ds_read like STRIDE);  v_cmpx narrows EXEC to the candidates' lanes (a NaN
// pace compares false, as above).  Under the narrowed mask:  thr = min(ceil(dl), 2^31),  row += STRIDE in place.  Then EXEC
// goes back to the saved mask.  6 VALU instructions for 7 (reference width: 5 for 6): the zeroing replaces one select, the
// other select and the copy of `row` the compiler makes when the read is left to it are gone.  A non-candidate fetches the
// word of the next attempt, or one row past the plane, as above.
// EXEC is saved once per statement, only ever narrowed from the saved mask (v_cmpx only clears bits) and back at its entry
// value when the statement ends: the compiler never sees a changed mask, and a lane that is off at entry (it has left
// the pass loop) stays off.  v_cmpx writes VCC as well on gfx9: clobbered, never read.  Wait states: VALU after a v_cmpx
// write of EXEC is interlocked, as is the scalar write of EXEC (see ovt_commit* below; no DPP, lane access or EXECZ /
// VCCZ operand here); od comes in an SGPR pair written by the scalar unit long before.
// THE LOAD IS HIDDEN FROM THE COMPILER: it counts no LDS operation for the statement and emits no s_waitcnt for `ow`.
//   * WAIT = true (the last pair of a pass's stage) ends the statement with s_waitcnt lgkmcnt(0).  LDS operations of a
//     wave return in order, so that one wait covers every word fetched by the stage's statements before it; it sits ahead
//     of everything that follows the stage: the branch out of the pass when no lane has a candidate (whose dead word
//     registers the allocator may hand out again at once -- a late return would land on their new contents), the paths
//     that overwrite the words with zeros, and the first commit that reads them.
//   * Between a statement and that wait the compiler's own code must not read or copy a word register: it is free to, as
//     far as it knows.  Checked in the assembly of the kernel's stage -- the stage's code between
//     statements is pace arithmetic on other registers -- and to be checked again when the stage changes.
//   * The compiler's own s_waitcnt lgkmcnt(n) for the pace gathers of the stage stay correct: the fetches it does not
//     count are younger than the gathers it waits for, so its counts are only conservative.
//   * volatile with a "memory" clobber: the stores of the two Philox blocks into the W plane stay ahead of the fetches,
//     and the statements stay in order.
template <uint32_t STRIDE, uint32_t OW, bool CEIL = true, bool WAIT = false>
__device__ __forceinline__ void ovt_threshold_x(double dl, double od, uint32_t &row, uint32_t &thr, uint32_t &ow)
{
    static_assert(OW <= 0xFFFFu, "the W plane's base must fit the 16-bit offset of a ds_read");
    uint64_t ex;
#define MCGP_THR_HEAD                                                                                                   \
    "s_mov_b64 %[ex], exec\n\t"                                                                                         \
    "v_mov_b32 %[thr], 0\n\t"                                                                                           \
    "ds_read_b32 %[ow], %[row] offset:%[base]\n\t"                                                                      \
    "v_cmpx_lt_f64 vcc, %[od], %[dl]\n\t"
#define MCGP_THR_TAIL                                                                                                   \
    "v_min_u32 %[thr], 0x80000000, %[thr]\n\t"                                                                          \
    "v_add_u32 %[row], %[stride], %[row]\n\t"                                                                           \
    "s_mov_b64 exec, %[ex]"
#define MCGP_THR_WAIT "\n\ts_waitcnt lgkmcnt(0)"
    if constexpr (CEIL) {
        double t;
        if constexpr (WAIT)
            asm volatile(MCGP_THR_HEAD "v_ceil_f64 %[t], %[dl]\n\tv_cvt_u32_f64 %[thr], %[t]\n\t" MCGP_THR_TAIL MCGP_THR_WAIT
                         : [thr] "=&v"(thr), [ow] "=&v"(ow), [row] "+v"(row), [t] "=&v"(t), [ex] "=&s"(ex)
                         : [dl] "v"(dl), [od] "s"(od), [stride] "n"(STRIDE), [base] "n"(OW)
                         : "vcc", "memory");
        else
            asm volatile(MCGP_THR_HEAD "v_ceil_f64 %[t], %[dl]\n\tv_cvt_u32_f64 %[thr], %[t]\n\t" MCGP_THR_TAIL
                         : [thr] "=&v"(thr), [ow] "=&v"(ow), [row] "+v"(row), [t] "=&v"(t), [ex] "=&s"(ex)
                         : [dl] "v"(dl), [od] "s"(od), [stride] "n"(STRIDE), [base] "n"(OW)
                         : "vcc", "memory");
    } else {
        if constexpr (WAIT)
            asm volatile(MCGP_THR_HEAD "v_cvt_u32_f64 %[thr], %[dl]\n\t" MCGP_THR_TAIL MCGP_THR_WAIT
                         : [thr] "=&v"(thr), [ow] "=&v"(ow), [row] "+v"(row), [ex] "=&s"(ex)
                         : [dl] "v"(dl), [od] "s"(od), [stride] "n"(STRIDE), [base] "n"(OW)
                         : "vcc", "memory");
        else
            asm volatile(MCGP_THR_HEAD "v_cvt_u32_f64 %[thr], %[dl]\n\t" MCGP_THR_TAIL
                         : [thr] "=&v"(thr), [ow] "=&v"(ow), [row] "+v"(row), [ex] "=&s"(ex)
                         : [dl] "v"(dl), [od] "s"(od), [stride] "n"(STRIDE), [base] "n"(OW)
                         : "vcc", "memory");
    }
#undef MCGP_THR_WAIT
#undef MCGP_THR_TAIL
#undef MCGP_THR_HEAD
}

// ---- overtake commits under EXEC ----
// The write-back chain of an overtake pass (reference :523-531): per adjacent pair (ahead, behind) with draw word w and
// threshold t, a success (w < t) sets  behind = ahead - 0.1,  ahead = behind + 0.3,  each rounded once, and the next pair
// sees the result.  A value that is computed and then kept or dropped needs no selects: v_cmpx narrows EXEC to the lanes
// whose attempt succeeded, the two additions write in place under it, and the scalar unit -- not the bottleneck -- ORs the
// pair's hits (VCC: v_cmpx writes both) into `acc` and restores EXEC.  3 VALU instructions per pair instead of 7.
// EXEC is saved once per statement and is back at its entry value when the statement ends: the compiler never sees a
// changed mask.  A lane that is off at entry (it has left the pass loop) stays off throughout -- v_cmpx only clears
// bits -- and contributes 0 to `acc`.  Wait states: an ordinary VALU instruction takes its lane mask from EXEC
// interlocked, whoever wrote it (the manual's EXEC hazards are DPP, v_readlane / v_writelane and EXECZ / VCCZ as data,
// none of which is here); the scalar reads of VCC and the scalar writes of EXEC are interlocked too.  -0.1 and 0.3
// come in SGPR pairs (VOP3 has no literals on gfx9).  Several pairs per statement for the reason given above.
#define MCGP_OVT_PAIR(a, b, w, t)                                                                                       \
    "v_cmpx_lt_u32 vcc, %[" #w "], %[" #t "]\n\t"                                                                       \
    "v_add_f64 %[" #b "], %[" #a "], %[dn]\n\t"                                                                         \
    "v_add_f64 %[" #a "], %[" #b "], %[up]\n\t"                                                                         \
    "s_or_b64 %[acc], %[acc], vcc\n\t"                                                                                  \
    "s_mov_b64 exec, %[ex]\n\t"
#define MCGP_OVT_CONSTS [dn] "s"(-0.1), [up] "s"(0.3)

__device__ __forceinline__ void ovt_commit1(double &c0, double &c1, uint32_t w1, uint32_t t1, uint64_t &acc)
{
    uint64_t ex;
    asm volatile("s_mov_b64 %[ex], exec\n\t"
                 MCGP_OVT_PAIR(c0, c1, w1, t1)
                 : [c0] "+v"(c0), [c1] "+v"(c1), [acc] "+s"(acc), [ex] "=&s"(ex)
                 : [w1] "v"(w1), [t1] "v"(t1), MCGP_OVT_CONSTS
                 : "vcc");
}
__device__ __forceinline__ void ovt_commit2(double &c0, double &c1, double &c2, uint32_t w1, uint32_t t1, uint32_t w2, uint32_t t2,
                                            uint64_t &acc)
{
    uint64_t ex;
    asm volatile("s_mov_b64 %[ex], exec\n\t"
                 MCGP_OVT_PAIR(c0, c1, w1, t1)
                 MCGP_OVT_PAIR(c1, c2, w2, t2)
                 : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [acc] "+s"(acc), [ex] "=&s"(ex)
                 : [w1] "v"(w1), [t1] "v"(t1), [w2] "v"(w2), [t2] "v"(t2), MCGP_OVT_CONSTS
                 : "vcc");
}
__device__ __forceinline__ void ovt_commit3(double &c0, double &c1, double &c2, double &c3, uint32_t w1, uint32_t t1, uint32_t w2,
                                            uint32_t t2, uint32_t w3, uint32_t t3, uint64_t &acc)
{
    uint64_t ex;
    asm volatile("s_mov_b64 %[ex], exec\n\t"
                 MCGP_OVT_PAIR(c0, c1, w1, t1)
                 MCGP_OVT_PAIR(c1, c2, w2, t2)
                 MCGP_OVT_PAIR(c2, c3, w3, t3)
                 : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3), [acc] "+s"(acc), [ex] "=&s"(ex)
                 : [w1] "v"(w1), [t1] "v"(t1), [w2] "v"(w2), [t2] "v"(t2), [w3] "v"(w3), [t3] "v"(t3), MCGP_OVT_CONSTS
                 : "vcc");
}
__device__ __forceinline__ void ovt_commit4(double &c0, double &c1, double &c2, double &c3, double &c4, uint32_t w1, uint32_t t1,
                                            uint32_t w2, uint32_t t2, uint32_t w3, uint32_t t3, uint32_t w4, uint32_t t4, uint64_t &acc)
{
    uint64_t ex;
    asm volatile("s_mov_b64 %[ex], exec\n\t"
                 MCGP_OVT_PAIR(c0, c1, w1, t1)
                 MCGP_OVT_PAIR(c1, c2, w2, t2)
                 MCGP_OVT_PAIR(c2, c3, w3, t3)
                 MCGP_OVT_PAIR(c3, c4, w4, t4)
                 : [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3), [c4] "+v"(c4), [acc] "+s"(acc), [ex] "=&s"(ex)
                 : [w1] "v"(w1), [t1] "v"(t1), [w2] "v"(w2), [t2] "v"(t2), [w3] "v"(w3), [t3] "v"(t3), [w4] "v"(w4), [t4] "v"(t4),
                   MCGP_OVT_CONSTS
                 : "vcc");
}
#undef MCGP_OVT_CONSTS
#undef MCGP_OVT_PAIR
// this lane's bit of the hits accumulated by the commits of a pass: one VOP3 select on the SGPR pair
__device__ __forceinline__ bool ovt_lane_hit(uint64_t acc)
{
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(acc));
    return r != 0u;
}

// ---- lap-step commits under EXEC ----
// What a car's lap changes (reference :179-223, :450-492), for 1..4 consecutive slots in time-rank order.  Per slot, with
// the old pk word p, the driver's LAST value `last` (its sign: the car retires on this lap) and `lt` holding the clean
// lap time at entry:
//   dirty  (p & DIRTY):                  lt = max(|carry|, lt + pen)       the lap time: clean-air cars keep the clean time
//   active (!(p & DNF)):                 carry = last                      (after this slot has read it)
//   run    (active, last >= 0):          cum += lt;  pk += 1 << AGE        (not on a lane that stops)
//   pit    (run, window, agef >= pitw):  cum += pit_loss;  pk = (p & ~(comp | used | age)) | fit
//   retire (active, last < 0):           pk = (p & ~age) | retire_word
// Nothing is computed for every lane and then selected: the compares go into SGPR pairs, the scalar unit -- not the
// bottleneck -- combines them, and each write is issued in place under EXEC = saved & mask, as in ovt_commit*.  The two
// additions to the time round in the order the select form had ((cum + lt) + pit_loss), a car that does not run keeps its
// bits (the select form added +0.0, the identity: no cumulative time is -0.0), and both pit and retirement words are
// built from the OLD p: a stopping lane is taken out of the age increment rather than masked afterwards.
// The mask sets alternate between two groups of SGPR pairs (x: even slots, z: odd) so that the compares of slot k + 1
// are issued before the writes of slot k wait for slot k's scalar results; a group of compares therefore opens by putting
// EXEC back to the saved mask (the writes before it have left it narrowed: a compare writes 0 for a lane that is off).
// EXEC is saved once and is back at its entry value at the end; every narrowing is saved & mask, so a lane that is off
// at entry stays off (v_cmp also writes 0 for such a lane).  Wait states, by producer / consumer pair:
//   v_cmp (VOP3) writes an SGPR pair -> s_and_b64 / s_xor_b64 reads it: a scalar read of a VALU-written SGPR is
//     interlocked (the manual's cases are v_readlane / v_writelane lane selects, v_div_fmas and VMEM, none here); no VALU
//     instruction of the statement reads an SGPR that a VALU instruction wrote: the masks reach the VALU only as EXEC.
//   s_and_b64 writes EXEC -> VALU: interlocked (see ovt_commit*; no DPP, lane access or EXECZ / VCCZ operand here).
//   No select remains, and VCC is not touched: there is no v_cmp -> VOP2 select pair to space.
//   pen, pit_loss and the two field masks come in SGPRs written by the scalar unit long before (lap constants).
#define MCGP_STEP_TEST(k, g)                                                                                            \
    "s_mov_b64 exec, %[ex]\n\t"                                                                                         \
    "v_and_b32 %[t], %[dnf], %[p" #k "]\n\t"                                                                            \
    "v_cmp_eq_u32 %[a" #g "], 0, %[t]\n\t"                                                                              \
    "v_cmp_gt_i32 %[d" #g "], 0, %[h" #k "]\n\t"                                                                        \
    "v_and_b32 %[t], %[dty], %[p" #k "]\n\t"                                                                            \
    "v_cmp_ge_u32 %[c" #g "], %[g" #k "], %[w" #k "]\n\t"                                                               \
    "v_cmp_ne_u32 %[y" #g "], 0, %[t]\n\t"
// The pit writes behind a branch.  A stop is decided by tyre age against a per-(compound, driver) threshold, so the 64
// races of a wave stop on the same few laps: at 20 cars some lane of the wave stops in one slot visit in eight (DESIGN
// 3.3j), yet the two pit writes and the fetch of the word a stop leaves were issued for every slot of every lap.  In the
// form below (StepSlot) the wave jumps over them:  s_and_b64 c, c, win leaves SCC = (c != 0) and s_cbranch_scc0 skips the
// pit region -- the address of the rule word from the OLD p and the lap's rule row (`lut`, an SGPR), its ds_read_b32, the
// time's second addition, s_waitcnt lgkmcnt(0) and the pk write.  s_xor a, a, c (a stopping lane leaves the age increment)
// is inside as well: with c = 0 it changes nothing.  (The retirement write stays on the common path: a branch over it
// costs more than the write at 2 and at 4 waves per SIMD, profiles/step_rare_bench.txt.)
// Every mask and every value is computed exactly as in the form without a branch (StepSlotFit, kept for the field sizes of
// reg_step_plain(): the word fetched ahead of the statement for every slot, every write issued); the time's first addition
// moves ahead of the pit mask's two ANDs so that nothing scalar sits between the AND that sets SCC and the branch.  The
// mask is an AND with compares that wrote 0 for a lane that is off: a lane off at entry never makes the wave enter the region.
// Wait states and the compiler's view, in addition to the list above:
//   s_and_b64 writes SCC -> s_cbranch_scc0 reads it: scalar to scalar, interlocked; no scalar instruction in between.
//   s_and_b64 writes EXEC -> v_and_b32 / ds_read_b32 (LDS takes its lanes from EXEC): interlocked, as for the VALU above.
//   THE FETCH IS HIDDEN FROM THE COMPILER, which counts no LDS operation for the statement.  The word lives in a statement
//     temporary ("=&v") that is dead when the region ends, and the region waits with s_waitcnt lgkmcnt(0) before it reads
//     it: whatever the compiler has in flight at entry has then returned as well (LDS returns in order), so every count it
//     emits after the statement is conservative-correct on both paths -- on the path that skips nothing was added, on the
//     path that fetches nothing is left.  The address sits in `t`, which no compare of a later slot reads before writing.
//     The rule rows are written once, before the block's first barrier, and never again: no "memory" clobber.
//   EXEC: set only to saved & mask inside the region, and back at the saved mask on both paths at the statement's end (a
//     region that is skipped leaves EXEC as the instruction ahead of its branch set it, which the next s_and_b64 replaces).
//   The branch target is a local label, unique per expansion of the statement (%=) and per slot.
#define MCGP_STEP_WRITE_HEAD(k, g)                                                                                      \
    "s_and_b64 exec, %[ex], %[y" #g "]\n\t"                                                                             \
    "v_add_f64 %[l" #k "], %[l" #k "], %[pen]\n\t"                                                                      \
    "v_max_f64 %[l" #k "], |%[cy]|, %[l" #k "]\n\t"                                                                     \
    "s_and_b64 exec, %[ex], %[a" #g "]\n\t"                                                                             \
    "v_mov_b64 %[cy], %[s" #k "]\n\t"                                                                                   \
    "s_and_b64 %[d" #g "], %[a" #g "], %[d" #g "]\n\t"                                                                  \
    "s_xor_b64 %[a" #g "], %[a" #g "], %[d" #g "]\n\t"
#define MCGP_STEP_WRITE_FIT(k, g)                                                                                       \
    MCGP_STEP_WRITE_HEAD(k, g)                                                                                          \
    "s_and_b64 %[c" #g "], %[c" #g "], %[a" #g "]\n\t"                                                                  \
    "s_and_b64 %[c" #g "], %[c" #g "], %[win]\n\t"                                                                      \
    "s_and_b64 exec, %[ex], %[a" #g "]\n\t"                                                                             \
    "v_add_f64 %[u" #k "], %[u" #k "], %[l" #k "]\n\t"                                                                  \
    "s_xor_b64 %[a" #g "], %[a" #g "], %[c" #g "]\n\t"                                                                  \
    "s_and_b64 exec, %[ex], %[c" #g "]\n\t"                                                                             \
    "v_add_f64 %[u" #k "], %[u" #k "], %[pl]\n\t"                                                                       \
    "v_and_or_b32 %[p" #k "], %[p" #k "], %[mpit], %[f" #k "]\n\t"                                                      \
    "s_and_b64 exec, %[ex], %[a" #g "]\n\t"                                                                             \
    "v_add_u32 %[p" #k "], %[age1], %[p" #k "]\n\t"                                                                     \
    "s_and_b64 exec, %[ex], %[d" #g "]\n\t"                                                                             \
    "v_and_or_b32 %[p" #k "], %[p" #k "], %[mage], %[rw]\n\t"
#define MCGP_STEP_WRITE_RARE(k, g)                                                                                      \
    MCGP_STEP_WRITE_HEAD(k, g)                                                                                          \
    "s_and_b64 exec, %[ex], %[a" #g "]\n\t"                                                                             \
    "v_add_f64 %[u" #k "], %[u" #k "], %[l" #k "]\n\t"                                                                  \
    "s_and_b64 %[c" #g "], %[c" #g "], %[a" #g "]\n\t"                                                                  \
    "s_and_b64 %[c" #g "], %[c" #g "], %[win]\n\t"                                                                      \
    "s_cbranch_scc0 .Lmcgp_step_run" #k "_%=\n\t"                                                                       \
    "s_xor_b64 %[a" #g "], %[a" #g "], %[c" #g "]\n\t"                                                                  \
    "s_and_b64 exec, %[ex], %[c" #g "]\n\t"                                                                             \
    "v_and_b32 %[t], %[used], %[p" #k "]\n\t"                                                                           \
    "v_lshl_add_u32 %[t], %[t], 2, %[lut]\n\t"                                                                          \
    "ds_read_b32 %[f], %[t]\n\t"                                                                                        \
    "v_add_f64 %[u" #k "], %[u" #k "], %[pl]\n\t"                                                                       \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                                          \
    "v_and_or_b32 %[p" #k "], %[p" #k "], %[mpit], %[f]\n"                                                              \
    ".Lmcgp_step_run" #k "_%=:\n\t"                                                                                     \
    "s_and_b64 exec, %[ex], %[a" #g "]\n\t"                                                                             \
    "v_add_u32 %[p" #k "], %[age1], %[p" #k "]\n\t"                                                                     \
    "s_and_b64 exec, %[ex], %[d" #g "]\n\t"                                                                             \
    "v_and_or_b32 %[p" #k "], %[p" #k "], %[mage], %[rw]\n\t"
#define MCGP_STEP_OUT(k) [p##k] "+v"(pk[k]), [u##k] "+v"(cum[k]), [l##k] "+v"(lt[k])
#define MCGP_STEP_IN(k)                                                                                                 \
    [h##k] "v"((uint32_t)__double2hiint(s[k].last)), [s##k] "v"(s[k].last), [g##k] "v"(s[k].agef), [w##k] "v"(s[k].pitw)
#define MCGP_STEP_IN_FIT(k) MCGP_STEP_IN(k), [f##k] "v"(s[k].fit)
#define MCGP_STEP_ENTER "s_mov_b64 %[ex], exec\n\ts_mov_b32 %[mpit], %[kpit]\n\ts_mov_b32 %[mage], %[kret]\n\t"
#define MCGP_STEP_LEAVE "s_mov_b64 exec, %[ex]"
// the order of the slots: the compares of slot k + 1 ahead of the writes of slot k (W: the write form)
#define MCGP_STEP_BODY1(W) MCGP_STEP_ENTER MCGP_STEP_TEST(0, x) W(0, x) MCGP_STEP_LEAVE
#define MCGP_STEP_BODY2(W) MCGP_STEP_ENTER MCGP_STEP_TEST(0, x) MCGP_STEP_TEST(1, z) W(0, x) W(1, z) MCGP_STEP_LEAVE
#define MCGP_STEP_BODY3(W) MCGP_STEP_ENTER MCGP_STEP_TEST(0, x) MCGP_STEP_TEST(1, z) W(0, x) MCGP_STEP_TEST(2, x) W(1, z) W(2, x) MCGP_STEP_LEAVE
#define MCGP_STEP_BODY4(W)                                                                                              \
    MCGP_STEP_ENTER MCGP_STEP_TEST(0, x) MCGP_STEP_TEST(1, z) W(0, x) MCGP_STEP_TEST(2, x) W(1, z) MCGP_STEP_TEST(3, z) W(2, x) W(3, z)   \
        MCGP_STEP_LEAVE
#define MCGP_STEP_TEMPS_X [t] "=&v"(t), [ex] "=&s"(ex), [mpit] "=&s"(mpit), [mage] "=&s"(mage), [ax] "=&s"(ax), [dx] "=&s"(dx), [cx] "=&s"(cx), [yx] "=&s"(yx)
#define MCGP_STEP_TEMPS_Z , [az] "=&s"(az), [dz] "=&s"(dz), [cz] "=&s"(cz), [yz] "=&s"(yz)
#define MCGP_STEP_TEMPS_RARE , [f] "=&v"(f)
#define MCGP_STEP_COMMON                                                                                                \
    [rw] "v"(c.retire_word), [win] "s"(c.window), [pl] "s"(c.pit_loss), [pen] "s"(c.pen), [kpit] "n"(KEEP_PIT),           \
        [kret] "n"(KEEP_RET), [dnf] "n"(DNF), [dty] "n"(DIRTY), [age1] "n"(AGE1)
#define MCGP_STEP_COMMON_RARE MCGP_STEP_COMMON, [lut] "s"(c.lut), [used] "n"(kStepUsed)
// one slot's inputs that are not updated in place
struct StepSlot {
    double last;         // the driver's LAST value: the last lap time, negative iff the car retires on this lap
    uint32_t agef;       // the age field of p, in place
    uint32_t pitw;       // pit threshold, positioned as the age field
};
// ... with the word a stop leaves fetched for every slot: selects the form without branches
struct StepSlotFit : StepSlot {
    uint32_t fit;        // compound and used-set a stop on this lap leaves, positioned as in pk
};
// the lap's wave-uniform inputs (SGPRs) and the retirement word (a VGPR: v_and_or_b32 takes one scalar operand)
struct StepLap {
    uint32_t retire_word;
    uint64_t window;     // all ones while the pit window is open, 0 otherwise
    double pit_loss, pen;
    uint32_t lut;        // byte address of the lap's row of the pit rule: the word a stop leaves, by used-set (StepSlot only)
};
constexpr uint32_t kStepUsed = 7u;           // the used-set bits of pk ([0..2]), the word index into that row
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit1(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlotFit *s, const StepLap &c)
{
    uint32_t t, mpit, mage;
    uint64_t ex, ax, dx, cx, yx;
    asm volatile(MCGP_STEP_BODY1(MCGP_STEP_WRITE_FIT)
                 : MCGP_STEP_OUT(0), [cy] "+v"(carry), MCGP_STEP_TEMPS_X
                 : MCGP_STEP_IN_FIT(0), MCGP_STEP_COMMON
                 : "scc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit1(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlot *s, const StepLap &c)
{
    uint32_t t, f, mpit, mage;
    uint64_t ex, ax, dx, cx, yx;
    asm volatile(MCGP_STEP_BODY1(MCGP_STEP_WRITE_RARE)
                 : MCGP_STEP_OUT(0), [cy] "+v"(carry), MCGP_STEP_TEMPS_X MCGP_STEP_TEMPS_RARE
                 : MCGP_STEP_IN(0), MCGP_STEP_COMMON_RARE
                 : "scc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit2(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlotFit *s, const StepLap &c)
{
    uint32_t t, mpit, mage;
    uint64_t ex, ax, dx, cx, yx, az, dz, cz, yz;
    asm volatile(MCGP_STEP_BODY2(MCGP_STEP_WRITE_FIT)
                 : MCGP_STEP_OUT(0), MCGP_STEP_OUT(1), [cy] "+v"(carry), MCGP_STEP_TEMPS_X MCGP_STEP_TEMPS_Z
                 : MCGP_STEP_IN_FIT(0), MCGP_STEP_IN_FIT(1), MCGP_STEP_COMMON
                 : "scc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit2(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlot *s, const StepLap &c)
{
    uint32_t t, f, mpit, mage;
    uint64_t ex, ax, dx, cx, yx, az, dz, cz, yz;
    asm volatile(MCGP_STEP_BODY2(MCGP_STEP_WRITE_RARE)
                 : MCGP_STEP_OUT(0), MCGP_STEP_OUT(1), [cy] "+v"(carry), MCGP_STEP_TEMPS_X MCGP_STEP_TEMPS_Z MCGP_STEP_TEMPS_RARE
                 : MCGP_STEP_IN(0), MCGP_STEP_IN(1), MCGP_STEP_COMMON_RARE
                 : "scc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit3(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlotFit *s, const StepLap &c)
{
    uint32_t t, mpit, mage;
    uint64_t ex, ax, dx, cx, yx, az, dz, cz, yz;
    asm volatile(MCGP_STEP_BODY3(MCGP_STEP_WRITE_FIT)
                 : MCGP_STEP_OUT(0), MCGP_STEP_OUT(1), MCGP_STEP_OUT(2), [cy] "+v"(carry), MCGP_STEP_TEMPS_X MCGP_STEP_TEMPS_Z
                 : MCGP_STEP_IN_FIT(0), MCGP_STEP_IN_FIT(1), MCGP_STEP_IN_FIT(2), MCGP_STEP_COMMON
                 : "scc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit3(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlot *s, const StepLap &c)
{
    uint32_t t, f, mpit, mage;
    uint64_t ex, ax, dx, cx, yx, az, dz, cz, yz;
    asm volatile(MCGP_STEP_BODY3(MCGP_STEP_WRITE_RARE)
                 : MCGP_STEP_OUT(0), MCGP_STEP_OUT(1), MCGP_STEP_OUT(2), [cy] "+v"(carry), MCGP_STEP_TEMPS_X MCGP_STEP_TEMPS_Z MCGP_STEP_TEMPS_RARE
                 : MCGP_STEP_IN(0), MCGP_STEP_IN(1), MCGP_STEP_IN(2), MCGP_STEP_COMMON_RARE
                 : "scc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit4(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlotFit *s, const StepLap &c)
{
    uint32_t t, mpit, mage;
    uint64_t ex, ax, dx, cx, yx, az, dz, cz, yz;
    asm volatile(MCGP_STEP_BODY4(MCGP_STEP_WRITE_FIT)
                 : MCGP_STEP_OUT(0), MCGP_STEP_OUT(1), MCGP_STEP_OUT(2), MCGP_STEP_OUT(3), [cy] "+v"(carry),
                   MCGP_STEP_TEMPS_X MCGP_STEP_TEMPS_Z
                 : MCGP_STEP_IN_FIT(0), MCGP_STEP_IN_FIT(1), MCGP_STEP_IN_FIT(2), MCGP_STEP_IN_FIT(3), MCGP_STEP_COMMON
                 : "scc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET>
__device__ __forceinline__ void step_commit4(double *cum, uint32_t *pk, double *lt, double &carry, const StepSlot *s, const StepLap &c)
{
    uint32_t t, f, mpit, mage;
    uint64_t ex, ax, dx, cx, yx, az, dz, cz, yz;
    asm volatile(MCGP_STEP_BODY4(MCGP_STEP_WRITE_RARE)
                 : MCGP_STEP_OUT(0), MCGP_STEP_OUT(1), MCGP_STEP_OUT(2), MCGP_STEP_OUT(3), [cy] "+v"(carry),
                   MCGP_STEP_TEMPS_X MCGP_STEP_TEMPS_Z MCGP_STEP_TEMPS_RARE
                 : MCGP_STEP_IN(0), MCGP_STEP_IN(1), MCGP_STEP_IN(2), MCGP_STEP_IN(3), MCGP_STEP_COMMON_RARE
                 : "scc");
}
#undef MCGP_STEP_COMMON_RARE
#undef MCGP_STEP_COMMON
#undef MCGP_STEP_TEMPS_RARE
#undef MCGP_STEP_TEMPS_Z
#undef MCGP_STEP_TEMPS_X
#undef MCGP_STEP_BODY4
#undef MCGP_STEP_BODY3
#undef MCGP_STEP_BODY2
#undef MCGP_STEP_BODY1
#undef MCGP_STEP_LEAVE
#undef MCGP_STEP_ENTER
#undef MCGP_STEP_IN_FIT
#undef MCGP_STEP_IN
#undef MCGP_STEP_OUT
#undef MCGP_STEP_WRITE_RARE
#undef MCGP_STEP_WRITE_FIT
#undef MCGP_STEP_WRITE_HEAD
#undef MCGP_STEP_TEST

// ---- position update under EXEC ----
// _update_positions (reference :538-560) for 1..4 consecutive slots in time-rank order, for a field WITHOUT equal times
// (update_positions_reg<N, true>, race_kernel_reg.hip.h).  Threaded through the slots, and from one statement to the
// next: `leader` and `prev` (the time of the first running car and of the last running car so far) and `first`, the
// lanes that have not met a running car yet (an SGPR pair).  Per slot, with time t and pk word p:
//   A = !(p & DNF)  (the car runs);   p &= ~(DRS | DIRTY)
//   under first:                                 leader = t   (it stops moving at the first running car: A leaves `first` below)
//   under ~first,      where t - leader < thr:   p |= DIRTY
//   under ~first & drs, where t - prev < 1.0:    p |= DRS
//   under A:  prev = t;   first &= ~A
// Nothing is merged by selects: `leader` and `prev` are moved in place under the lanes they change for, and each flag is
// OR-ed in under EXEC narrowed first to the lanes that may get it and then, by v_cmpx, to the lanes whose gap is below the
// bound.  Both subtractions are the select form's, rounded once; `thr > tbl` is the C++ `tbl < thr` (a compare does not
// round, no time is NaN).  For a field without equal times "not the first running car" stands in for :552's 0 < gap, as
// in update_positions_reg<N, true>.  A retired car's two flags come out as the arithmetic leaves them, as in the select
// form: nothing reads them.  FIRST: the statement opens the field -- every lane is still looking for its first running
// car at slot 0, which therefore gets no flag and hands its time to `leader` and to `prev` (a lane whose slot 0 is
// retired reads neither before the first running car has replaced both), and `first` is written, not read.
// The running tests of all slots and the clearing of the flags open the statement under the saved mask, so that a slot
// itself changes EXEC four times and no compare result has to be kept: six SGPR pairs besides the inputs.  EXEC is saved
// once, only ever set to a subset of the saved mask (saved & mask, or narrowed further by v_cmpx, which only clears bits),
// and back at its entry value at the end: a lane that is off at entry stays off and nothing of it is written.
// Wait states, by producer / consumer pair:
//   v_cmp (VOP3) writes an SGPR pair -> s_and_b64 / s_andn2_b64 reads it: interlocked, as in step_commit* above; no VALU
//     instruction reads an SGPR a VALU instruction of the statement wrote (VCC is written by v_cmpx and never read).
//   s_and_b64 / v_cmpx writes EXEC -> VALU: interlocked (see ovt_commit*; no DPP, lane access or EXECZ / VCCZ operand).
//   thr comes in an SGPR pair written before the statement (scalar_f64: at least three VALU instructions earlier), the
//     DRS lanes in one the scalar unit reads.
#define MCGP_UPD_ENTER "s_mov_b64 %[ex], exec\n\ts_and_b64 %[xd], %[ex], %[drm]\n\t"
#define MCGP_UPD_HEAD(k)                                                                                                \
    "v_and_b32 %[t], %[dnf], %[p" #k "]\n\t"                                                                            \
    "v_and_b32 %[p" #k "], %[clr], %[p" #k "]\n\t"                                                                      \
    "v_cmp_eq_u32 %[a" #k "], 0, %[t]\n\t"
#define MCGP_UPD_SLOT(k)                                                                                                \
    "s_and_b64 exec, %[ex], %[f]\n\t"                                                                                   \
    "v_mov_b64 %[ld], %[u" #k "]\n\t"                                                                                   \
    "s_andn2_b64 exec, %[ex], %[f]\n\t"                                                                                 \
    "v_add_f64 %[tb], %[u" #k "], -%[ld]\n\t"                                                                           \
    "v_add_f64 %[gp], %[u" #k "], -%[pv]\n\t"                                                                           \
    "v_cmpx_gt_f64 vcc, %[thr], %[tb]\n\t"                                                                              \
    "v_or_b32 %[p" #k "], %[dty], %[p" #k "]\n\t"                                                                       \
    "s_andn2_b64 exec, %[xd], %[f]\n\t"                                                                                 \
    "v_cmpx_gt_f64 vcc, 1.0, %[gp]\n\t"                                                                                 \
    "v_or_b32 %[p" #k "], %[drs], %[p" #k "]\n\t"                                                                       \
    "s_and_b64 exec, %[ex], %[a" #k "]\n\t"                                                                             \
    "v_mov_b64 %[pv], %[u" #k "]\n\t"                                                                                   \
    "s_andn2_b64 %[f], %[f], %[a" #k "]\n\t"
#define MCGP_UPD_SLOT_FIRST                                                                                             \
    "v_mov_b64 %[ld], %[u0]\n\t"                                                                                        \
    "v_mov_b64 %[pv], %[u0]\n\t"                                                                                        \
    "s_andn2_b64 %[f], %[ex], %[a0]\n\t"
#define MCGP_UPD_LEAVE "s_mov_b64 exec, %[ex]"
#define MCGP_UPD_BODY1(S0) MCGP_UPD_ENTER MCGP_UPD_HEAD(0) S0 MCGP_UPD_LEAVE
#define MCGP_UPD_BODY2(S0) MCGP_UPD_ENTER MCGP_UPD_HEAD(0) MCGP_UPD_HEAD(1) S0 MCGP_UPD_SLOT(1) MCGP_UPD_LEAVE
#define MCGP_UPD_BODY3(S0) MCGP_UPD_ENTER MCGP_UPD_HEAD(0) MCGP_UPD_HEAD(1) MCGP_UPD_HEAD(2) S0 MCGP_UPD_SLOT(1) MCGP_UPD_SLOT(2) MCGP_UPD_LEAVE
#define MCGP_UPD_BODY4(S0)                                                                                              \
    MCGP_UPD_ENTER MCGP_UPD_HEAD(0) MCGP_UPD_HEAD(1) MCGP_UPD_HEAD(2) MCGP_UPD_HEAD(3) S0 MCGP_UPD_SLOT(1) MCGP_UPD_SLOT(2)   \
        MCGP_UPD_SLOT(3) MCGP_UPD_LEAVE
#define MCGP_UPD_SLOT_OPS(k) [p##k] "+v"(pk[k]), [a##k] "=&s"(a[k])
#define MCGP_UPD_STATE [ld] "+v"(leader), [pv] "+v"(prev), [f] "+s"(first), [t] "=&v"(t), [tb] "=&v"(tb), [gp] "=&v"(gp), [ex] "=&s"(ex), [xd] "=&s"(xd)
#define MCGP_UPD_COMMON [thr] "s"(c.thr), [drm] "s"(c.drs), [dnf] "n"(DNF), [dty] "n"(DIRTY), [drs] "n"(DRS), [clr] "n"(~(DIRTY | DRS))
#define MCGP_UPD_TEMPS                                                                                                  \
    uint32_t t;                                                                                                         \
    double tb, gp;                                                                                                      \
    uint64_t ex, xd, a[4]
// the lap's wave-uniform inputs (SGPR pairs)
struct UpdLap {
    double thr;          // dirty-air threshold
    uint64_t drs;        // the lanes whose race has DRS enabled on this lap
};
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
__device__ __forceinline__ void upd_commit1(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    MCGP_UPD_TEMPS;
    if constexpr (FIRST)
        asm volatile(MCGP_UPD_BODY1(MCGP_UPD_SLOT_FIRST)
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_STATE : [u0] "v"(cum[0]), MCGP_UPD_COMMON : "scc", "vcc");
    else
        asm volatile(MCGP_UPD_BODY1(MCGP_UPD_SLOT(0))
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_STATE : [u0] "v"(cum[0]), MCGP_UPD_COMMON : "scc", "vcc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
__device__ __forceinline__ void upd_commit2(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    MCGP_UPD_TEMPS;
    if constexpr (FIRST)
        asm volatile(MCGP_UPD_BODY2(MCGP_UPD_SLOT_FIRST)
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_SLOT_OPS(1), MCGP_UPD_STATE
                     : [u0] "v"(cum[0]), [u1] "v"(cum[1]), MCGP_UPD_COMMON : "scc", "vcc");
    else
        asm volatile(MCGP_UPD_BODY2(MCGP_UPD_SLOT(0))
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_SLOT_OPS(1), MCGP_UPD_STATE
                     : [u0] "v"(cum[0]), [u1] "v"(cum[1]), MCGP_UPD_COMMON : "scc", "vcc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
__device__ __forceinline__ void upd_commit3(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    MCGP_UPD_TEMPS;
    if constexpr (FIRST)
        asm volatile(MCGP_UPD_BODY3(MCGP_UPD_SLOT_FIRST)
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_SLOT_OPS(1), MCGP_UPD_SLOT_OPS(2), MCGP_UPD_STATE
                     : [u0] "v"(cum[0]), [u1] "v"(cum[1]), [u2] "v"(cum[2]), MCGP_UPD_COMMON : "scc", "vcc");
    else
        asm volatile(MCGP_UPD_BODY3(MCGP_UPD_SLOT(0))
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_SLOT_OPS(1), MCGP_UPD_SLOT_OPS(2), MCGP_UPD_STATE
                     : [u0] "v"(cum[0]), [u1] "v"(cum[1]), [u2] "v"(cum[2]), MCGP_UPD_COMMON : "scc", "vcc");
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
__device__ __forceinline__ void upd_commit4(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    MCGP_UPD_TEMPS;
    if constexpr (FIRST)
        asm volatile(MCGP_UPD_BODY4(MCGP_UPD_SLOT_FIRST)
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_SLOT_OPS(1), MCGP_UPD_SLOT_OPS(2), MCGP_UPD_SLOT_OPS(3), MCGP_UPD_STATE
                     : [u0] "v"(cum[0]), [u1] "v"(cum[1]), [u2] "v"(cum[2]), [u3] "v"(cum[3]), MCGP_UPD_COMMON : "scc", "vcc");
    else
        asm volatile(MCGP_UPD_BODY4(MCGP_UPD_SLOT(0))
                     : MCGP_UPD_SLOT_OPS(0), MCGP_UPD_SLOT_OPS(1), MCGP_UPD_SLOT_OPS(2), MCGP_UPD_SLOT_OPS(3), MCGP_UPD_STATE
                     : [u0] "v"(cum[0]), [u1] "v"(cum[1]), [u2] "v"(cum[2]), [u3] "v"(cum[3]), MCGP_UPD_COMMON : "scc", "vcc");
}
#undef MCGP_UPD_TEMPS
#undef MCGP_UPD_COMMON
#undef MCGP_UPD_STATE
#undef MCGP_UPD_SLOT_OPS
#undef MCGP_UPD_BODY4
#undef MCGP_UPD_BODY3
#undef MCGP_UPD_BODY2
#undef MCGP_UPD_BODY1
#undef MCGP_UPD_LEAVE
#undef MCGP_UPD_SLOT_FIRST
#undef MCGP_UPD_SLOT
#undef MCGP_UPD_HEAD
#undef MCGP_UPD_ENTER
// the lanes of the wavefront in which the predicate holds (an SGPR pair), and the mask with every lane in it
__device__ __forceinline__ uint64_t lane_mask(bool pred) { return __ballot(pred); }
constexpr uint64_t kAllLanes = ~0ull;

// LDS access by ABSOLUTE byte address.  The register kernel declares no static __shared__ data, so its
// dynamic LDS block starts at address 0 (checked once at kernel entry); addressing it by number instead of
// through the `extern __shared__` symbol lets the compiler fold every table / row base into the 16-bit
// immediate offset of the ds_read / ds_write instead of adding the (symbolic) base in a VALU instruction.
#define MCGP_LDS __attribute__((address_space(3)))
template <typename T>
__device__ __forceinline__ T lds_ld(uint32_t addr)
{
    return *reinterpret_cast<const MCGP_LDS T *>(addr);
}
template <typename T>
__device__ __forceinline__ void lds_st(uint32_t addr, T v)
{
    *reinterpret_cast<MCGP_LDS T *>(addr) = v;
}
// OR into a word of LDS without reading it back: one ds_or_b32, nothing to wait for
__device__ __forceinline__ void lds_or_u32(uint32_t addr, uint32_t bits)
{
    (void)__hip_atomic_fetch_or(reinterpret_cast<MCGP_LDS uint32_t *>(addr), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ float4 lds_ld_float4(uint32_t addr)          // one ds_read_b128
{
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f v = *reinterpret_cast<const MCGP_LDS v4f *>(addr);
    return make_float4(v.x, v.y, v.z, v.w);
}
struct f64x2 {
    double x, y;
};
__device__ __forceinline__ f64x2 lds_ld_f64x2(uint32_t addr)             // one ds_read_b128 (16-byte aligned address)
{
    typedef double v2d __attribute__((ext_vector_type(2)));
    const v2d v = *reinterpret_cast<const MCGP_LDS v2d *>(addr);
    return f64x2{v.x, v.y};
}
// 16-byte stores / loads of two doubles or four words (16-byte aligned address)
__device__ __forceinline__ void lds_st_f64x2(uint32_t addr, double a, double b)
{
    typedef double v2d __attribute__((ext_vector_type(2)));
    v2d v;
    v.x = a;
    v.y = b;
    *reinterpret_cast<MCGP_LDS v2d *>(addr) = v;
}
__device__ __forceinline__ void lds_st_u32x4(uint32_t addr, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v4u v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    *reinterpret_cast<MCGP_LDS v4u *>(addr) = v;
}
__device__ __forceinline__ void lds_ld_u32x4(uint32_t addr, uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u v = *reinterpret_cast<const MCGP_LDS v4u *>(addr);
    a = v.x; b = v.y; c = v.z; d = v.w;
}
// {f64, u32, u32}: one ds_read_b128 (16-byte aligned address)
__device__ __forceinline__ void lds_ld_f64_u32x2(uint32_t addr, double &d, uint32_t &u0, uint32_t &u1)
{
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const v4u v = *reinterpret_cast<const MCGP_LDS v4u *>(addr);
    d = __hiloint2double((int)v.y, (int)v.x);
    u0 = v.z;
    u1 = v.w;
}

// Two doubles 16 bytes apart at BASE + addr: one ds_read2_b64, offsets BASE / 8 and BASE / 8 + 2 (8-bit fields in units of
// 8 bytes; the compiler pairs two loads off one address register whose offsets fit them)
template <uint32_t BASE>
__device__ __forceinline__ void lds_ld2_f64(uint32_t addr, double &a, double &b)
{
    static_assert(BASE % 8 == 0 && BASE / 8 + 2 <= 255, "ds_read2_b64 offsets");
    a = lds_ld<double>(BASE + addr);
    b = lds_ld<double>(BASE + 16u + addr);
}

// binary64 -> uint32 the way the hardware converts: toward zero, saturating at 0 and 2^32 - 1, NaN -> 0.
// (A C++ cast is undefined outside the range; the draw-word thresholds of the overtake step rely on the clamp.)
__device__ __forceinline__ uint32_t cvt_u32_f64_sat(double x)
{
    uint32_t r;
    asm("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ double ceil_f64(double x) { return __builtin_ceil(x); }
__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
// scheduling fence: the compiler's instruction scheduler moves nothing across it
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }
// ---- cross-lane pieces of the cooperative event handler ----
// LDS written by some lanes of the wave, read by others: program order is enough for the hardware (DS operations of
// one wave execute in order); this keeps the compiler from moving LDS accesses across the hand-over.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double readlane_f64(double x, int lane)       // lane: wave-uniform
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double bpermute_f64(double x, int src_lane)   // src_lane: per lane
{
    const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(x));
    return __hiloint2double(hi, lo);
}
// The wave's next work ticket: one lane takes it from the launch's counter in device memory, every lane gets the
// value (wave-uniform).  `turn` and `waves` are for the host emulation, whose threads run one after another.
__device__ __forceinline__ uint32_t next_ticket(uint32_t *counter, uint32_t /*tid*/, uint32_t /*turn*/, int /*waves*/)
{
    uint32_t t = 0u;
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u)
        t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
}
// a ticket counter's current value, without taking a ticket
__device__ __forceinline__ uint32_t peek_ticket(const uint32_t *counter)
{
    return __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the first lane of the wavefront in which the predicate holds, 64 if there is none (wave-uniform result)
__device__ __forceinline__ uint32_t first_lane_with(bool pred)
{
    const unsigned long long m = __ballot(pred);
    return m ? (uint32_t)__builtin_ctzll(m) : 64u;
}
// true if the predicate holds in ANY lane of the wavefront (wave-uniform result)
#define MCGP_ANY(pred) (__any((int)(pred)) != 0)
// Keeps a value computed where it is written: the compiler may not sink its computation into one arm of a later
// select and turn the select into a branch (no instruction is emitted).
__device__ __forceinline__ void pin(uint32_t &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void pin(double &x) { asm volatile("" : "+v"(x)); }
// the same for a wave-uniform value (an SGPR)
__device__ __forceinline__ void pin_scalar(uint32_t &x) { asm volatile("" : "+s"(x)); }
// a wave-uniform pointer the optimiser cannot see through: loads through it stay where they are written
template <typename T>
__device__ __forceinline__ void pin_ptr(const T *&p) { asm volatile("" : "+s"(p)); }
// A load from device memory at `base` (wave-uniform) + `off` bytes (per lane), said to be global: a pointer that went
// through pin_ptr has lost its address space, and a flat load through it pays 64-bit vector address arithmetic where
// the global one takes the base in scalar registers and the offset as it is.
#define MCGP_GLOBAL __attribute__((address_space(1)))
template <typename T>
__device__ __forceinline__ T global_ld(const void *base, uint32_t off)
{
    return *(const MCGP_GLOBAL T *)((const MCGP_GLOBAL unsigned char *)base + off);
}

// address of the dynamic LDS block as the hardware sees it
__device__ __forceinline__ uint32_t lds_base_of(const void *p)
{
    return (uint32_t)(uintptr_t)(const MCGP_LDS void *)p;
}

}  // namespace mcgp
#endif
