// retire_table_main.cpp -- stand-alone check of the retirement table (csrc/params_build.h: build_retire_table) and of the
// search in it (csrc/race_common.hip.h: retirement_lap_from_table) against the chain of draw_retirement_lap, as host
// code with its own main (tests/test_retirement_table_host.py builds it with the host's sanitizers and runs it).
//   table == chain, entry for entry, zeros behind it; search == draw_retirement_lap for the words 0, 2^32 - 1, every
//   S_k - 1, S_k, S_k + 1 and 10^5 random words, per-lap probabilities {0, 2^-32, 0.05/60, 0.01, 0.3, 0.5, 1 - 2^-32, 1},
//   L in {1, 2, 3, 4, 5, 60, 78, 129, 1000}; the same for the 64-bit chain of the reference-width kernel.
// Prints "ok" and returns 0, or names the first mismatch and returns 1.
#include "../../monte_carlo_gp_amd/csrc/params_build.h"

#include <cstdio>
#include <memory>
#include <vector>

namespace {

// the 64-bit chain as the reference-width kernel ran it per lane (and the oracle's philox_retirement_lap does):
// S_2 = q, S_{k+1} = floor(S_k q / 2^64); the lap (2 .. L) or 0
uint32_t draw_retirement_lap64(uint64_t w, uint64_t t, uint64_t q, int L)
{
    if (t == 0ull) return 0u;
    uint64_t S = q;
    for (int k = 2; k <= L; ++k) {
        if (!(w < S)) return (uint32_t)k;
        S = (uint64_t)(((unsigned __int128)S * q) >> 64);
    }
    return 0u;
}

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next_random()                       // splitmix64
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr int kRandomWords = 100000;

template <typename T>
int check_width(const mcgp::KParams &kp, const double *probs, bool wide, int random_words)
{
    const int L = kp.total_laps, n = kp.n;
    const size_t bytes = mcgp::retire_table_bytes(n, L, wide), row = mcgp::retire_row_entries(L);
    // exactly the bytes the builder is promised: a write or a read past them is the sanitizer's to report
    std::unique_ptr<T[]> tab(new T[bytes / sizeof(T)]);
    if (bytes != (size_t)mcgp::retire_table_rows(n) * row * sizeof(T) || row < (size_t)(L > 1 ? L : 1)) {
        std::printf("L %d: table of %zu bytes, rows of %zu entries\n", L, bytes, row);
        return 1;
    }
    mcgp::build_retire_table(kp, wide, tab.get());
    for (uint32_t d = 0; d < mcgp::retire_table_rows(n); ++d) {
        const T *S = tab.get() + (size_t)d * row;
        const bool live = d < (uint32_t)n && kp.t_dnf[d] != 0ull;
        const T q = !live ? (T)0 : wide ? (T)kp.q64_dnf[d] : (T)(4294967296ull - kp.t_dnf[d]);
        // table == chain
        T s = q;
        for (size_t i = 0; i < row; ++i) {
            const T want = live && i + 2 <= (size_t)L ? s : (T)0;
            if (S[i] != want) {
                std::printf("width %d L %d driver %u entry %zu: table %llu, chain %llu\n", wide ? 64 : 32, L, d, i,
                            (unsigned long long)S[i], (unsigned long long)want);
                return 1;
            }
            if (i > 0 && S[i] > S[i - 1]) {
                std::printf("width %d L %d driver %u: the row increases at entry %zu\n", wide ? 64 : 32, L, d, i);
                return 1;
            }
            s = wide ? (T)(((unsigned __int128)s * q) >> 64) : (T)mcgp::retire_next_threshold((uint32_t)s, (uint32_t)q);
        }
        if (!live) continue;                                       // p = 0: no row to search, the kernels skip the driver
        // search == chain
        std::vector<T> words = {(T)0, (T)~(T)0};
        for (int k = 2; k <= L; ++k)
            for (int e = -1; e <= 1; ++e) words.push_back((T)(S[k - 2] + (T)e));       // (wraps at both ends: still words)
        for (int i = 0; i < random_words; ++i) words.push_back((T)next_random());
        for (const T w : words) {
            const uint32_t got = mcgp::retirement_lap_from_table<T>(w, S, L);
            const uint32_t want = wide ? draw_retirement_lap64((uint64_t)w, kp.t_dnf[d], kp.q64_dnf[d], L)
                                       : mcgp::draw_retirement_lap((uint32_t)w, kp.t_dnf[d], L);
            if (got != want) {
                std::printf("width %d L %d p %.17g word %llu: search %u, chain %u\n", wide ? 64 : 32, L, probs[d],
                            (unsigned long long)w, got, want);
                return 1;
            }
        }
    }
    return 0;
}

}  // namespace

int main()
{
    const double probs[] = {0.0, 0x1p-32, 0.05 / 60.0, 0.01, 0.3, 0.5, 1.0 - 0x1p-32, 1.0};
    const int laps[] = {1, 2, 3, 4, 5, 60, 78, 129, 1000};
    constexpr int n = (int)(sizeof(probs) / sizeof(probs[0]));
    static mcgp::KParams kp;
    for (const int L : laps) {
        // 7 drivers of the 8 in a second pass (boundary words only), so that the table has a padding row as well
        for (int drop = 0; drop < 2; ++drop) {
            std::memset(&kp, 0, sizeof(kp));
            kp.n = n - drop;
            kp.total_laps = L;
            for (int d = 0; d < kp.n; ++d) {
                kp.t_dnf[d] = mcgp::threshold(probs[d]);
                kp.q64_dnf[d] = mcgp::survival64(probs[d]);
            }
            const int words = drop ? 0 : kRandomWords;
            if (check_width<uint32_t>(kp, probs, false, words) || check_width<uint64_t>(kp, probs, true, words)) return 1;
        }
    }
    // the largest table the library makes room for
    if (mcgp::retire_table_bytes(mcgp::kMaxCars, mcgp::kMaxLaps, true) > mcgp::kRetireTabMaxBytes) {
        std::printf("kRetireTabMaxBytes is too small\n");
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
