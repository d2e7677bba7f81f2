// cmpx_bench.hip -- what a (time, payload) compare-exchange costs on gfx950, by form.  Not product code.
//   A  the kernel's form (race_isa.hip.h cmpx_time): v_cmp_gt_f64 vcc; v_min_f64; v_max_f64; 2 x v_cndmask_b32 (payload)
//   B  v_cmpx_gt_f64 (EXEC := the lanes that swap); 3 x v_swap_b32 (time low, time high, payload); s_mov_b64 exec, saved
//   C  v_cmp_gt_f64 vcc; s_and_b64 exec, saved, vcc; 3 x v_swap_b32; s_mov_b64 exec, saved
//   S  the write-back chain of an overtake pass by selects: v_cmp_lt_u32 vcc; 2 x v_add_f64; 4 x v_cndmask_b32; s_or_b64 (hit lanes)
//   E  the same under EXEC (race_isa.hip.h ovt_commit*): v_cmpx_lt_u32; 2 x v_add_f64 in place; s_or_b64; s_mov_b64 exec, saved
//      (S and E as chains of 15 dependent pairs only; "comparator" in the output is then one pair)
//   LS the lap step's commit of four consecutive slots by selects (the carry, the dirty-air lap time, the time and the pk word: 3
//      compares, 2 shifts + 4 ands, 8 selects, a two-entry LDS read)
//   LE the same under EXEC (race_isa.hip.h step_commit4): 4 compares into SGPR pairs, each write in place under saved & mask
//      ("comparator" in the output is one slot; both include the same clean-time and age-field instructions and loop overhead)
//   US the position update of four consecutive slots by selects (update_positions_reg<N, true> as compiled: leader, prev and the two
//      flag bits merged by 6 selects, the running test twice, 3 ands, 2 subtractions, 2 binary64 compares, a v_or3)
//   UE the same under EXEC (race_isa.hip.h upd_commit4<.., false>): leader and prev moved in place, each flag OR-ed in under EXEC
//      narrowed by a mask and then by v_cmpx;  UF with slot 0 opening the field (upd_commit4<.., true>)
//      (per slot; lanes with a retired car in front of the first running one, with one between two running ones, with DRS off)
//   TS the threshold stage of an overtake pass by selects (race_isa.hip.h ovt_threshold): per adjacent pair a binary64 compare, ceil,
//      convert, min, add, 2 x v_cndmask_b32 and the read of the pair's draw word from the W plane; a chain of 19 pairs
//   TE the same under EXEC (race_isa.hip.h ovt_threshold_x): threshold zeroed, word read, v_cmpx, then ceil, convert, min and the row
//      advance in place on the candidates' lanes; EXEC saved and restored per pair.  TE4: four pairs to a statement (EXEC saved once
//      per four).  TE4Z: TE4 with two thresholds zeroed by one v_mov_b64.  (per pair; 5 pairs in 32 are candidates, lane by lane)
//   LF.. the lap step's commit of four slots with the rare writes behind a branch (race_isa.hip.h step_commit*): LF the sequence
//      without a branch (rule-word fetch for every slot, pit and retirement writes always issued), LFS a branch per slot over
//      the pit region (fetch, wait and both writes inside), LFB one branch per batch of four over all four pit regions, LFR a
//      branch per slot over the retirement write, LFSR / LFBR both; at r0 / r13 / r100: 0 %, 13 % and 100 % of slot visits have a
//      stopping lane, 4.7 % a retiring one (tools/cmpx_bench_gen.py says how).  The forms of one rate print equal check values.
//      tools/cmpx_bench LF runs these alone (any argument: the cases whose name starts with it).  Their bodies are generated
//      where the benchmark is built (python3 tools/cmpx_bench_gen.py step > tools/cmpx_step_bodies.inc); without that file
//      the benchmark builds without them
// each as layers of 8 independent comparators (the sorting network) and as a chain of 15 dependent ones (a bubble pass).
// The loop bodies are written on fixed registers (v[10:41] = 16 times, v50..v65 = 16 payloads): inline assembly cannot
// name the halves of a 64-bit operand, which form B needs.
//   python3 tools/cmpx_bench_gen.py step > tools/cmpx_step_bodies.inc
//   hipcc --offload-arch=gfx950 -O3 -o tools/cmpx_bench tools/cmpx_bench.hip && tools/cmpx_bench
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// the kernels: tools/cmpx_bench_gen.py > tools/cmpx_bodies.inc
#include "cmpx_bodies.inc"
#if __has_include("cmpx_step_bodies.inc")
#include "cmpx_step_bodies.inc"
#define CMPX_STEP_FORMS 1
#endif

struct Case { const char *name; void (*fn)(uint32_t, double *); int comparators; };

int main(int argc, char **argv)
{
    const std::string only = argc > 1 ? argv[1] : "";
    const Case cases[] = {{"A layers (cmp, min, max, 2 cndmask + 3 moves)", k_A_layer, 16}, {"A0 layers (the 3 moves alone)", k_A0_layer, 16},
                          {"B layers (cmpx, 3 swaps, restore)", k_B_layer, 16}, {"C layers (cmp, s_and exec, 3 swaps, restore)", k_C_layer, 16},
                          {"D layers (cmpx, payload swap, restore, min, max + 2 moves)", k_D_layer, 16},
                          {"A chain", k_A_chain, 15}, {"A0 chain", k_A0_chain, 15}, {"B chain", k_B_chain, 15}, {"C chain", k_C_chain, 15},
                          {"D chain", k_D_chain, 15},
                          {"S chain (overtake commit: cmp, 2 add, 4 cndmask)", k_S_chain, 15},
                          {"E chain (overtake commit: cmpx, 2 add in place, restore)", k_E_chain, 15},
                          {"LS (lap-step commit of 4 slots by selects; per slot)", k_LS_chain, 4},
                          {"LE (lap-step commit of 4 slots under EXEC; per slot)", k_LE_chain, 4},
                          {"US (position update of 4 slots by selects; per slot)", k_US_chain, 4},
                          {"UE (position update of 4 slots under EXEC; per slot)", k_UE_chain, 4},
                          {"UF (the same, slot 0 opening the field; per slot)", k_UF_chain, 4},
                          {"TS (overtake thresholds of 19 pairs by selects; per pair)", k_TS_chain, 19},
                          {"TE (overtake thresholds under EXEC, a pair to a statement; per pair)", k_TE_chain, 19},
                          {"TE4 (the same, four pairs to a statement; per pair)", k_TE4_chain, 19},
                          {"TE4Z (TE4, thresholds zeroed two at a time; per pair)", k_TE4Z_chain, 19},
#ifdef CMPX_STEP_FORMS
#define STEPF(form, what)                                                                                               \
    {#form " r0 (" what "; no stop; per slot)", k_##form##_r0_chain, 4}, {#form " r13 (" what "; 13 % stops; per slot)", k_##form##_r13_chain, 4},   \
    {#form " r100 (" what "; 100 % stops; per slot)", k_##form##_r100_chain, 4}
                          STEPF(LF, "no branch"), STEPF(LFS, "pit branch per slot"), STEPF(LFB, "pit branch per batch"),
                          STEPF(LFR, "retirement branch"), STEPF(LFSR, "pit per slot + retirement"),
                          STEPF(LFBR, "pit per batch + retirement"),
#undef STEPF
#endif
    };
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    double *out;
    CHECK(hipMalloc(&out, 64 * sizeof(double) * 16));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const uint32_t iters = 40000;
    for (int W = 2; W <= 4; ++W) {
        for (const Case &c : cases) {
            if (std::string(c.name).compare(0, only.size(), only) != 0) continue;
            // W blocks of 256 threads per CU (LDS reservation keeps it at W)
            const size_t lds = 160 * 1024 / W - 1024;
            CHECK(hipFuncSetAttribute((const void *)c.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(c.fn, dim3(cus * W), dim3(256), lds, 0, 1000u, out);
            CHECK(hipDeviceSynchronize());
            CHECK(hipEventRecord(e0));
            hipLaunchKernelGGL(c.fn, dim3(cus * W), dim3(256), lds, 0, iters, out);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            double h[64], sum = 0.0;       // (every block writes the same 64 values: one per lane)
            CHECK(hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost));
            for (double x : h) sum += x;
            const double cyc = 1024.0 * 2.4e9 * ms * 1e-3 / ((double)cus * 4 * W * iters * c.comparators);
            printf("waves/SIMD %d  %-56s %.2f cycles per comparator per SIMD   (check %.3f %.3f, all lanes %.3f)\n", W, c.name, cyc, h[0], h[5], sum);
        }
    }
    return 0;
}
