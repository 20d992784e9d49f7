// Stand-alone bounds check of tmg_trace's kernels (csrc/tmg_trace.hip) on the
// host wave emulator: `make trace_asan` builds it with AddressSanitizer and
// UBSan.  n in {1, 3} envs, seqs in {1, 2} action rows (row 0 the lowest
// effective action of each env, row 1 uniform, so mostly ineffective, with one
// negative action), max_frames in {1, 4}, all stages selected, stop = 0, with
// and without `frames`, on a shape whose frames are written as bytes (2N = 126)
// and one whose frames are written as words; every array is a heap block of
// exactly its rows, so the sanitizer sees any load or store past them.  Each
// row's sums, flags and RNG words are compared with one emu_step (autoreset
// off) on a one-env copy, and so is its last frame when the move fits
// max_frames.
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
    std::mt19937_64 g(5);
    const int shapes[][4] = {{7, 9, 5, 15}, {10, 10, 4, 14}};
    const int moves = 30;
    const uint32_t all = 0x7Eu;
    long checked = 0, framed = 0;
    for (auto &sh : shapes) {
        const int R = sh[0], C = sh[1], k = sh[2], sm = sh[3], N = R * C, A = 2 * N - R - C, W = (A + 63) / 64;
        for (int64_t n : {1, 3}) {
            auto board = block<int8_t>((size_t)n * 2 * N, 0);
            auto rng = block<uint64_t>(n * 5, 0), eff = block<uint64_t>(n * W, 0);
            auto timer = block<int32_t>(n, 0);
            assert(emu_seed(n, 0, nullptr, 1, 200, 0, 0, 0, 0, rng.get()) == 0);
            assert(emu_reset(R, C, k, sm, moves, n, board.get(), rng.get(), timer.get(), eff.get()) == 0);
            for (int Q : {1, 2}) {
                const int64_t m = n * Q;
                auto acts = block<int32_t>(m, 0);
                for (int64_t j = 0; j < m; j++) acts[j] = (int32_t)(g() % (uint64_t)A);
                for (int64_t i = 0; i < n; i++)
                    for (int a = 0; a < A; a++)
                        if ((eff[i * W + (a >> 6)] >> (a & 63)) & 1) { acts[i] = a; break; }
                if (Q > 1) acts[m - 1] = -1;
                for (int F : {1, 4})
                    for (int withf = 0; withf < 2; withf++) {
                        auto frames = block<int8_t>(withf ? (size_t)m * F * 2 * N : 1, 0x77);
                        auto kind = block<uint8_t>(m * F, 0x77);
                        auto fe = block<int32_t>(m * F, 0x77), nf = block<int32_t>(m, 0x77);
                        auto rew = block<int32_t>(m, 0x77), nn = block<int32_t>(m, 0x77), na = block<int32_t>(m, 0x77);
                        auto flags = block<uint8_t>(m, 0x77);
                        auto org = block<uint64_t>(m * 5, 0x77);
                        const int rc = emu_trace(R, C, k, sm, n, board.get(), rng.get(), eff.get(), 1, Q, acts.get(), all, F, 0,
                                                 withf ? frames.get() : nullptr, kind.get(), fe.get(), nf.get(), rew.get(),
                                                 nn.get(), na.get(), flags.get(), org.get());
                        if (rc) { fprintf(stderr, "trace refused: %d\n", rc); return 1; }
                        for (int64_t v = 0; v < m; v++) {
                            const int64_t i = v % n;
                            std::vector<int8_t> b1(board.get() + i * 2 * N, board.get() + (i + 1) * 2 * N);
                            uint64_t r1[5], e1[16];
                            memcpy(r1, rng.get() + i * 5, 40);
                            memcpy(e1, eff.get() + i * W, 8 * W);
                            int32_t t1 = 0, r = 0, n1 = 0, n2 = 0, a = acts[v];
                            uint8_t f1 = 0;
                            if (a >= 0)
                                emu_step(R, C, k, sm, moves, 1, b1.data(), r1, &t1, &a, &r, &n1, &n2, &f1, e1, 1, 0, 0, 0, 0, 0,
                                         nullptr, nullptr, nullptr, nullptr, nullptr);
                            bool ok = rew[v] == r && nn[v] == n1 && na[v] == n2 && flags[v] == (f1 & 0x86) &&
                                      !memcmp(org.get() + v * 5, r1, 40);
                            int sum = 0;
                            for (int f = 0; f < F; f++) {
                                const bool used = f < nf[v];
                                ok = ok && (used ? kind[v * F + f] >= 1 && kind[v * F + f] <= 6 : kind[v * F + f] == 0 && fe[v * F + f] == 0);
                                sum += fe[v * F + f];
                            }
                            if (nf[v] <= F) ok = ok && sum + nn[v] == rew[v];
                            if (withf) {
                                for (int f = nf[v] < F ? nf[v] : F; f < F; f++)
                                    for (int b = 0; b < 2 * N; b++) ok = ok && frames[((size_t)v * F + f) * 2 * N + b] == 0x77;
                                if (nf[v] > 0 && nf[v] <= F) {
                                    ok = ok && !memcmp(frames.get() + ((size_t)v * F + nf[v] - 1) * 2 * N, b1.data(), 2 * N);
                                    framed++;
                                }
                            }
                            if (!ok) {
                                fprintf(stderr, "row %ld of %dx%d n=%ld Q=%d F=%d differs from the stepped copy\n", (long)v, R, C,
                                        (long)n, Q, F);
                                return 1;
                            }
                            checked++;
                        }
                    }
            }
        }
    }
    if (emu_status() != 0) { fprintf(stderr, "status %u\n", emu_status()); return 1; }
    if (!framed) { fprintf(stderr, "no row's last frame was compared\n"); return 1; }
    printf("trace_asan ok: %ld rows checked\n", checked);
    return 0;
}
