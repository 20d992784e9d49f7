// Stand-alone bounds check of tmg_expand's count / scan and gather kernels
// (csrc/tmg_expand.hip) on the host wave emulator: `make expand_asan` builds it
// with AddressSanitizer and UBSan, and it runs both store variants of the
// gather over exactly sized heap buffers (synthetic boards and masks, select
// and none, m at, below and above the total) against a plain host loop.
#include "emu.cpp"
#include <random>
#include <memory>
#include <cassert>

int main() {
    std::mt19937_64 g(1);
    const int shapes[][2] = {{3, 5}, {4, 4}, {7, 9}, {10, 10}, {2, 64}, {20, 20}, {3, 43}, {1, 3}, {16, 16}};
    long checked = 0;
    for (auto &sh : shapes) {
        const int R = sh[0], C = sh[1], N = R * C, A = 2 * N - R - C, W = (A + 63) / 64, moves = 9;
        for (int64_t n : {1, 9, 70}) {
            for (int usesel = 0; usesel < 2; usesel++) {
                std::vector<int8_t> board((size_t)n * 2 * N);
                for (auto &b : board) b = (int8_t)(g() % 7);
                std::vector<uint64_t> rng(n * 5), eff(n * W), sel(n * W);
                for (auto &x : rng) x = g();
                for (auto &x : eff) x = g() & g();
                for (auto &x : sel) x = g();
                std::vector<int32_t> timer(n);
                for (auto &t : timer) t = (int32_t)(g() % 12);
                std::vector<int64_t> first(n + 1, -1);
                const uint64_t *sp = usesel ? sel.data() : nullptr;
                assert(emu_expand_count(R, C, moves, n, timer.data(), eff.data(), sp, first.data()) == 0);
                // reference
                std::vector<int64_t> par; std::vector<int> act;
                for (int64_t i = 0; i < n; i++) {
                    assert(first[i] == (int64_t)par.size());
                    if (timer[i] >= moves) continue;
                    for (int a = 0; a < A; a++) {
                        uint64_t w = eff[i * W + a / 64];
                        if (usesel) w &= sel[i * W + a / 64];
                        if ((w >> (a & 63)) & 1) { par.push_back(i); act.push_back(a); }
                    }
                }
                const int64_t total = (int64_t)par.size();
                assert(first[n] == total);
                for (int64_t m : {total, total - 3, total + 5, (int64_t)1}) {
                    if (m <= 0) continue;
                    for (int pack = 0; pack < 2; pack++) {
                        // exactly sized heap buffers: ASan sees any write past row m
                        std::unique_ptr<int8_t[]> cbv(new int8_t[(size_t)m * 2 * N]);
                        std::unique_ptr<uint64_t[]> cr(new uint64_t[m * 5]), ce(new uint64_t[m * W]);
                        std::unique_ptr<int32_t[]> ct(new int32_t[m]), ca(new int32_t[m]);
                        std::unique_ptr<int64_t[]> cp(new int64_t[m]);
                        memset(cbv.get(), 0x77, (size_t)m * 2 * N);
                        for (int64_t c = 0; c < m; c++) { ct[c] = -7; ca[c] = -7; cp[c] = -7; }
                        const tmg::ExpandArgs a{n, m, N, W, A, moves, board.data(), rng.data(), timer.data(), eff.data(), sp,
                                                first.data(), cbv.get(), cr.get(), ct.get(), ce.get(), cp.get(), ca.get()};
                        if (N <= 128) {
                            if (pack) run_blocks(n, 0, [&] { tmg::expand_gather_kernel<1, true>(a); });
                            else run_blocks(n, 0, [&] { tmg::expand_gather_kernel<1, false>(a); });
                        } else {
                            if (pack) run_blocks(n, 0, [&] { tmg::expand_gather_kernel<4, true>(a); });
                            else run_blocks(n, 0, [&] { tmg::expand_gather_kernel<4, false>(a); });
                        }
                        for (int64_t c = 0; c < m; c++) {
                            if (c < total) {
                                const int64_t i = par[c];
                                assert(cp[c] == i && ca[c] == act[c] && ct[c] == timer[i]);
                                assert(!memcmp(cbv.get() + c * 2 * N, board.data() + i * 2 * N, 2 * N));
                                assert(!memcmp(cr.get() + c * 5, rng.data() + i * 5, 40));
                                assert(!memcmp(ce.get() + c * W, eff.data() + i * W, 8 * W));
                            } else {
                                assert(cp[c] == -1 && ca[c] == 0 && ct[c] == moves);
                                for (int w = 0; w < W; w++) assert(ce[c * W + w] == 0);
                                for (int b = 0; b < 2 * N; b++) assert(cbv[c * 2 * N + b] == 0x77);
                            }
                            checked++;
                        }
                    }
                }
            }
        }
    }
    // count alone, several tiles
    for (int64_t n : {0, 1023, 1024, 1025, 70000}) {
        const int R = 10, C = 10, A = 180, W = 3;
        std::vector<uint64_t> eff(n * W + 1);
        std::vector<int32_t> timer(n + 1);
        for (auto &x : eff) x = g();
        for (auto &t : timer) t = (int32_t)(g() % 12);
        std::unique_ptr<int64_t[]> first(new int64_t[n + 1]);
        assert(emu_expand_count(R, C, 9, n, timer.data(), eff.data(), nullptr, first.get()) == 0);
        int64_t run = 0;
        for (int64_t i = 0; i < n; i++) {
            assert(first[i] == run);
            if (timer[i] < 9) run += __builtin_popcountll(eff[i * W]) + __builtin_popcountll(eff[i * W + 1]) +
                                     __builtin_popcountll(eff[i * W + 2] & ((1ULL << (A - 128)) - 1));
        }
        assert(first[n] == run);
    }
    printf("expand_asan ok: %ld child rows checked\n", checked);
    return 0;
}
