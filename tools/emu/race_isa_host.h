// Host stand-in for csrc/race_isa.hip.h (tools/emu only): same include guard, portable bodies.
#ifndef MCGP_RACE_ISA_H
#define MCGP_RACE_ISA_H
#include <hip/hip_runtime.h>
namespace mcgp {
inline void minmax_f64(double a, double b, double &lo, double &hi)
{
    lo = a < b ? a : b;       // times are finite, non-negative: identical to v_min_f64 / v_max_f64
    hi = a < b ? b : a;
}
inline double max_f64(double a, double b) { return a < b ? b : a; }
inline double max_abs_f64(double a, double b) { return std::fabs(a) < b ? b : std::fabs(a); }
inline void cmpx_time(double &ca, uint32_t &pa, double &cb, uint32_t &pb)
{
    if (ca > cb) {
        const double t = ca; ca = cb; cb = t;
        const uint32_t q = pa; pa = pb; pb = q;
    }
}
inline void cmpx_time2(double &a1, uint32_t &pa1, double &b1, uint32_t &pb1, double &a2, uint32_t &pa2, double &b2, uint32_t &pb2)
{
    cmpx_time(a1, pa1, b1, pb1);
    cmpx_time(a2, pa2, b2, pb2);
}
inline void bubble_fwd2(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2)
{
    cmpx_time(c0, p0, c1, p1);
    cmpx_time(c1, p1, c2, p2);
}
inline void bubble_bwd2(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2)
{
    cmpx_time(c1, p1, c2, p2);
    cmpx_time(c0, p0, c1, p1);
}
inline void bubble_fwd3(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3)
{
    cmpx_time(c0, p0, c1, p1);
    cmpx_time(c1, p1, c2, p2);
    cmpx_time(c2, p2, c3, p3);
}
inline void bubble_bwd3(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3)
{
    cmpx_time(c2, p2, c3, p3);
    cmpx_time(c1, p1, c2, p2);
    cmpx_time(c0, p0, c1, p1);
}
inline void bubble_fwd4(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3, double &c4, uint32_t &p4)
{
    cmpx_time(c0, p0, c1, p1);
    cmpx_time(c1, p1, c2, p2);
    cmpx_time(c2, p2, c3, p3);
    cmpx_time(c3, p3, c4, p4);
}
inline void bubble_bwd4(double &c0, uint32_t &p0, double &c1, uint32_t &p1, double &c2, uint32_t &p2, double &c3, uint32_t &p3, double &c4, uint32_t &p4)
{
    cmpx_time(c3, p3, c4, p4);
    cmpx_time(c2, p2, c3, p3);
    cmpx_time(c1, p1, c2, p2);
    cmpx_time(c0, p0, c1, p1);
}
// LDS by absolute byte address: the emulated LDS block is the array mcgp::smem
extern unsigned char smem[];
template <typename T>
inline T lds_ld(uint32_t addr)
{
    T v;
    std::memcpy(&v, smem + addr, sizeof(T));
    return v;
}
template <typename T>
inline void lds_st(uint32_t addr, T v)
{
    std::memcpy(smem + addr, &v, sizeof(T));
}
inline void lds_or_u32(uint32_t addr, uint32_t bits) { lds_st<uint32_t>(addr, lds_ld<uint32_t>(addr) | bits); }
struct f64x2 {
    double x, y;
};
inline f64x2 lds_ld_f64x2(uint32_t addr) { return lds_ld<f64x2>(addr); }
inline void lds_ld_f64_u32x2(uint32_t addr, double &d, uint32_t &u0, uint32_t &u1)
{
    d = lds_ld<double>(addr);
    u0 = lds_ld<uint32_t>(addr + 8);
    u1 = lds_ld<uint32_t>(addr + 12);
}
template <uint32_t BASE>
inline void lds_ld2_f64(uint32_t addr, double &a, double &b)
{
    a = lds_ld<double>(BASE + addr);
    b = lds_ld<double>(BASE + 16u + addr);
}
// v_cvt_u32_f64: toward zero, saturating, NaN -> 0
inline uint32_t cvt_u32_f64_sat(double x)
{
    if (!(x > 0.0)) return 0u;
    if (x >= 4294967295.0) return 0xFFFFFFFFu;
    return (uint32_t)x;
}
// the emulated threads run one after another: a wave's turn-th chunk is a fixed one
inline uint32_t next_ticket(uint32_t *, uint32_t tid, uint32_t turn, int waves) { return turn * (uint32_t)waves + tid / 64u; }
inline uint32_t peek_ticket(const uint32_t *counter) { return *counter; }
inline uint32_t first_lane_with(bool pred) { return pred ? 0u : 64u; }
inline void sched_fence() {}
inline double ceil_f64(double x) { return std::ceil(x); }
inline uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }
template <uint32_t STRIDE, bool CEIL = true>
inline void ovt_threshold(double dl, double od, uint32_t row, uint32_t &thr, uint32_t &next)
{
    const uint32_t stride = STRIDE;
    const bool c = dl > od;
    thr = c ? min_u32(cvt_u32_f64_sat(CEIL ? std::ceil(dl) : dl), 0x80000000u) : 0u;
    next = row + (c ? stride : 0u);
}
// the same pair with the word fetch inside (the device statement narrows EXEC; WAIT is its wait for the fetches)
template <uint32_t STRIDE, uint32_t OW, bool CEIL = true, bool WAIT = false>
inline void ovt_threshold_x(double dl, double od, uint32_t &row, uint32_t &thr, uint32_t &ow)
{
    const uint32_t stride = STRIDE;
    const bool c = dl > od;
    ow = lds_ld<uint32_t>(OW + row);
    thr = c ? min_u32(cvt_u32_f64_sat(CEIL ? std::ceil(dl) : dl), 0x80000000u) : 0u;
    row += c ? stride : 0u;
}
// overtake commits (reference :523-531): the portable loop body; `acc` is the one emulated lane's hit bit
inline void ovt_commit1(double &c0, double &c1, uint32_t w1, uint32_t t1, uint64_t &acc)
{
    const bool hit = w1 < t1;
    const double nb = c0 - 0.1;
    const double na = nb + 0.3;
    c1 = hit ? nb : c1;
    c0 = hit ? na : c0;
    acc |= hit ? 1u : 0u;
}
inline void ovt_commit2(double &c0, double &c1, double &c2, uint32_t w1, uint32_t t1, uint32_t w2, uint32_t t2, uint64_t &acc)
{
    ovt_commit1(c0, c1, w1, t1, acc);
    ovt_commit1(c1, c2, w2, t2, acc);
}
inline void ovt_commit3(double &c0, double &c1, double &c2, double &c3, uint32_t w1, uint32_t t1, uint32_t w2, uint32_t t2, uint32_t w3,
                        uint32_t t3, uint64_t &acc)
{
    ovt_commit2(c0, c1, c2, w1, t1, w2, t2, acc);
    ovt_commit1(c2, c3, w3, t3, acc);
}
inline void ovt_commit4(double &c0, double &c1, double &c2, double &c3, double &c4, uint32_t w1, uint32_t t1, uint32_t w2, uint32_t t2,
                        uint32_t w3, uint32_t t3, uint32_t w4, uint32_t t4, uint64_t &acc)
{
    ovt_commit3(c0, c1, c2, c3, w1, t1, w2, t2, w3, t3, acc);
    ovt_commit1(c3, c4, w4, t4, acc);
}
inline bool ovt_lane_hit(uint64_t acc) { return acc != 0u; }
// lap-step commits (reference :179-223, :450-492): the portable body of one slot, slots in order
struct StepSlot {
    double last;
    uint32_t agef, pitw;
};
struct StepSlotFit : StepSlot {
    uint32_t fit;
};
inline uint32_t step_fit(const StepSlot &, uint32_t p, uint32_t lut);
inline uint32_t step_fit(const StepSlotFit &s, uint32_t, uint32_t) { return s.fit; }
struct StepLap {
    uint32_t retire_word;
    uint64_t window;
    double pit_loss, pen;
    uint32_t lut;
};
constexpr uint32_t kStepUsed = 7u;
// fetched on a stop only, as on the device
inline uint32_t step_fit(const StepSlot &, uint32_t p, uint32_t lut) { return lds_ld<uint32_t>(((p & kStepUsed) << 2) + lut); }
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET, class Slot>
inline void step_commit1(double *cum, uint32_t *pk, double *lt, double &carry, const Slot *s, const StepLap &c)
{
    const uint32_t p = pk[0];
    const bool active = !(p & DNF);
    uint64_t bits;
    std::memcpy(&bits, &s[0].last, 8);
    const bool dnf_hit = (bits >> 63) != 0u;
    const bool run = active && !dnf_hit;
    const bool pit = run && c.window != 0u && s[0].agef >= s[0].pitw;
    if (p & DIRTY) lt[0] = max_abs_f64(carry, lt[0] + c.pen);
    if (active) carry = s[0].last;
    if (run) cum[0] = cum[0] + lt[0];
    if (pit) cum[0] = cum[0] + c.pit_loss;
    if (pit) pk[0] = (p & KEEP_PIT) | step_fit(s[0], p, c.lut);
    else if (run) pk[0] = p + AGE1;
    else if (active) pk[0] = (p & KEEP_RET) | c.retire_word;
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET, class Slot>
inline void step_commit2(double *cum, uint32_t *pk, double *lt, double &carry, const Slot *s, const StepLap &c)
{
    step_commit1<DNF, DIRTY, AGE1, KEEP_PIT, KEEP_RET>(cum, pk, lt, carry, s, c);
    step_commit1<DNF, DIRTY, AGE1, KEEP_PIT, KEEP_RET>(cum + 1, pk + 1, lt + 1, carry, s + 1, c);
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET, class Slot>
inline void step_commit3(double *cum, uint32_t *pk, double *lt, double &carry, const Slot *s, const StepLap &c)
{
    step_commit2<DNF, DIRTY, AGE1, KEEP_PIT, KEEP_RET>(cum, pk, lt, carry, s, c);
    step_commit1<DNF, DIRTY, AGE1, KEEP_PIT, KEEP_RET>(cum + 2, pk + 2, lt + 2, carry, s + 2, c);
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t AGE1, uint32_t KEEP_PIT, uint32_t KEEP_RET, class Slot>
inline void step_commit4(double *cum, uint32_t *pk, double *lt, double &carry, const Slot *s, const StepLap &c)
{
    step_commit3<DNF, DIRTY, AGE1, KEEP_PIT, KEEP_RET>(cum, pk, lt, carry, s, c);
    step_commit1<DNF, DIRTY, AGE1, KEEP_PIT, KEEP_RET>(cum + 3, pk + 3, lt + 3, carry, s + 3, c);
}
// position update of a field without equal times (reference :538-560): the portable body of one slot, slots in order;
// `first` and the DRS mask are the one emulated lane's bits
struct UpdLap {
    double thr;
    uint64_t drs;
};
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
inline void upd_commit1(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    const uint32_t p = pk[0];
    const bool act = !(p & DNF), fst = FIRST || first != 0u;       // (FIRST: slot 0 of the field, `first` is written only)
    const double t = cum[0];
    if (fst) leader = t;
    const double tbl = t - leader;
    const bool dirty = !fst && tbl < c.thr;
    const bool drs = !fst && c.drs != 0u && (t - prev) < 1.0;
    pk[0] = (p & ~(DRS | DIRTY)) | (dirty ? DIRTY : 0u) | (drs ? DRS : 0u);
    if (act || FIRST) prev = t;
    first = fst && !act ? 1u : 0u;
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
inline void upd_commit2(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    upd_commit1<DNF, DIRTY, DRS, FIRST>(cum, pk, leader, prev, first, c);
    upd_commit1<DNF, DIRTY, DRS, false>(cum + 1, pk + 1, leader, prev, first, c);
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
inline void upd_commit3(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    upd_commit2<DNF, DIRTY, DRS, FIRST>(cum, pk, leader, prev, first, c);
    upd_commit1<DNF, DIRTY, DRS, false>(cum + 2, pk + 2, leader, prev, first, c);
}
template <uint32_t DNF, uint32_t DIRTY, uint32_t DRS, bool FIRST>
inline void upd_commit4(const double *cum, uint32_t *pk, double &leader, double &prev, uint64_t &first, const UpdLap &c)
{
    upd_commit3<DNF, DIRTY, DRS, FIRST>(cum, pk, leader, prev, first, c);
    upd_commit1<DNF, DIRTY, DRS, false>(cum + 3, pk + 3, leader, prev, first, c);
}
inline uint64_t lane_mask(bool pred) { return pred ? 1u : 0u; }
constexpr uint64_t kAllLanes = 1u;
// threads of the emulated block run one after another: "any lane" is this thread alone (both paths behind an
// MCGP_ANY test compute the same results, so which one a thread takes does not matter); EMU_FORCE_ANY=1 sends every
// thread down the "some lane needs it" path, which a single-thread view would otherwise reach only rarely
#ifdef EMU_FORCE_ANY
#define MCGP_ANY(pred) ((void)(pred), true)
#else
#define MCGP_ANY(pred) (pred)
#endif
inline void pin(uint32_t &) {}
inline void pin(double &) {}
inline void pin_scalar(uint32_t &) {}
template <typename T>
inline void pin_ptr(const T *&) {}
template <typename T>
inline T global_ld(const void *base, uint32_t off)
{
    return *reinterpret_cast<const T *>(static_cast<const unsigned char *>(base) + off);
}
inline float4 lds_ld_float4(uint32_t addr) { return lds_ld<float4>(addr); }
inline uint32_t lds_base_of(const void *p) { return (uint32_t)((const unsigned char *)p - smem); }
}  // namespace mcgp
#endif
