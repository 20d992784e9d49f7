// Stand-alone bounds check of tmg_playout's kernels (csrc/tmg_playout.hip and
// the reduce kernel of csrc/tmg_aux.hip) on the host wave emulator: `make
// playout_asan` builds it with AddressSanitizer and UBSan.  n in {1, 3} envs,
// Q in {1, 3} sequences of D = 3 actions (uniform, so most are ineffective; one
// sequence is cut short by a negative action), with and without the
// final-state outputs, on a general shape of at most 128 cells and a lean one;
// every array is a heap block of exactly its rows, so the sanitizer sees any
// load or store past them.  Each row is compared with a plain host loop of
// emu_step calls (autoreset off) on a one-env copy.
#include "emu.cpp"
#include <cassert>
#include <memory>
#include <random>

template <class T>
static std::unique_ptr<T[]> block(size_t count, int fill) {
    std::unique_ptr<T[]> p(new T[count]);
    memset(p.get(), fill, count * sizeof(T));
    return p;
}

int main() {
    std::mt19937_64 g(3);
    const int shapes[][4] = {{7, 9, 5, 15}, {10, 10, 4, 0}};           // general (2N = 126: byte stores), lean
    const int moves = 30, D = 3;
    long checked = 0;
    for (auto &sh : shapes) {
        const int R = sh[0], C = sh[1], k = sh[2], sm = sh[3], N = R * C, A = 2 * N - R - C, W = (A + 63) / 64;
        for (int64_t n : {1, 3}) {
            // the parents: seeded, reset, with the library's own masks
            auto board = block<int8_t>((size_t)n * 2 * N, 0);
            auto rng = block<uint64_t>(n * 5, 0), eff = block<uint64_t>(n * W, 0);
            auto timer = block<int32_t>(n, 0);
            assert(emu_seed(n, 0, nullptr, 1, 100, 0, 0, 0, 0, rng.get()) == 0);
            assert(emu_reset(R, C, k, sm, moves, n, board.get(), rng.get(), timer.get(), eff.get()) == 0);
            for (int Q : {1, 3}) {
                const int64_t m = n * Q;
                auto acts = block<int32_t>(m * D, 0);
                for (int64_t j = 0; j < m * D; j++) acts[j] = (int32_t)(g() % (uint64_t)A);
                acts[(m - 1) * D + 1] = -1;                                  // the last sequence: one ply
                for (int fin = 0; fin < 2; fin++) {
                    auto ret = block<int32_t>(m, 0x77), nn = block<int32_t>(m, 0x77), na = block<int32_t>(m, 0x77);
                    auto plies = block<int32_t>(m, 0x77), ply = block<int32_t>(m * D, 0x77);
                    auto flags = block<uint8_t>(m, 0x77);
                    auto bs = block<int32_t>(n, 0x77), br = block<int32_t>(n, 0x77);
                    auto ob = block<int8_t>(fin ? (size_t)m * 2 * N : 1, 0x77);
                    auto org = block<uint64_t>(fin ? m * 5 : 1, 0x77), oe = block<uint64_t>(fin ? m * W : 1, 0x77);
                    auto ot = block<int32_t>(fin ? m : 1, 0x77);
                    const int rc = emu_playout(R, C, k, sm, moves, n, board.get(), rng.get(), 0, timer.get(), eff.get(), 1,
                                               Q, D, acts.get(), ret.get(), nn.get(), na.get(), plies.get(), flags.get(),
                                               ply.get(), fin ? ob.get() : nullptr, fin ? org.get() : nullptr,
                                               fin ? ot.get() : nullptr, fin ? oe.get() : nullptr, bs.get(), br.get());
                    if (rc) { fprintf(stderr, "playout refused: %d\n", rc); return 1; }
                    for (int64_t v = 0; v < m; v++) {
                        const int64_t i = v % n;
                        // the host loop: D steps of a one-env copy
                        std::vector<int8_t> b1(board.get() + i * 2 * N, board.get() + (i + 1) * 2 * N);
                        uint64_t r1[5], e1[16];
                        memcpy(r1, rng.get() + i * 5, 40);
                        memcpy(e1, eff.get() + i * W, 8 * W);
                        int32_t t1 = timer[i], rew = 0, n1 = 0, n2 = 0, sum = 0, s1 = 0, s2 = 0, np = 0;
                        uint8_t f1 = 0, fl = 0;
                        for (int d = 0; d < D; d++) {
                            int32_t a = acts[v * D + d];
                            if (a < 0) break;
                            emu_step(R, C, k, sm, moves, 1, b1.data(), r1, &t1, &a, &rew, &n1, &n2, &f1, e1, 1, 0, 0, 0, 0, 0,
                                     nullptr, nullptr, nullptr, nullptr, nullptr);
                            if (ply[v * D + d] != rew) { fprintf(stderr, "ply_reward differs: row %ld ply %d\n", (long)v, d); return 1; }
                            sum += rew; s1 += n1; s2 += n2; fl |= f1; np++;
                        }
                        bool ok = ret[v] == sum && nn[v] == s1 && na[v] == s2 && plies[v] == np && flags[v] == fl;
                        for (int d = np; d < D; d++) ok = ok && ply[v * D + d] == 0;
                        if (fin)
                            ok = ok && !memcmp(ob.get() + v * 2 * N, b1.data(), 2 * N) && !memcmp(org.get() + v * 5, r1, 40) &&
                                 !memcmp(oe.get() + v * W, e1, 8 * W) && ot[v] == t1;
                        if (!ok) { fprintf(stderr, "row %ld of %dx%d n=%ld Q=%d differs from the stepped copy\n", (long)v, R, C, (long)n, Q); return 1; }
                        checked++;
                    }
                    for (int64_t i = 0; i < n; i++) {
                        int best = 0;
                        for (int q = 1; q < Q; q++)
                            if (ret[q * n + i] > ret[best * n + i]) best = q;
                        if (bs[i] != best || br[i] != ret[best * n + i]) { fprintf(stderr, "best differs: env %ld\n", (long)i); return 1; }
                    }
                }
            }
        }
    }
    if (emu_status() != 0) { fprintf(stderr, "status %u\n", emu_status()); return 1; }
    printf("playout_asan ok: %ld rows checked\n", checked);
    return 0;
}
