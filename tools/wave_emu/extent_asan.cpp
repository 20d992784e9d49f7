// Stand-alone extent check of the wave-per-board kernels on the host wave
// emulator: `make extent_asan` builds it with AddressSanitizer and UBSan, and
// it runs reset, masked reset, steps in every autoreset mode with the five
// vector outputs attached (trusted, untrusted after a hand edit, in-kernel
// policy; num_moves = 2, so every second step ends every episode and the
// deferred or next-step reset regenerates every row), the same steps on rows
// [1, n) of the blocks (what a plan group is), peek, rollout and effective.
// Every array is an exactly sized heap block of n rows, so a load or a store
// outside rows 0..n-1 is an ASan report; rows outside a mask or a group must
// keep their bytes.  The shapes are tests/extent_cases.py EXTENT_SHAPES, at
// n = 1 and 9 (boards of <= 128 cells) and n = 1 and 3 (512-cell boards).
// The emulator has no lane kernel: the lane shapes run on the wave kernels.
// Values are not compared here (the emulated parity tests do that).
#include "emu.cpp"
#include <memory>
#include <random>

#include <sys/wait.h>
#include <unistd.h>

namespace {

constexpr int kMoves = 2;
constexpr uint64_t kKey = 4242;
constexpr int64_t kFirst = 1000;

[[noreturn]] void die(const char *what, const int *sh, int64_t n) {
    fprintf(stderr, "extent_asan: %s (%dx%d k%d s%d, n = %ld)\n", what, sh[0], sh[1], sh[2], sh[3], (long)n);
    exit(1);
}

// an exactly sized heap block of n rows of rb bytes
struct Arr {
    std::unique_ptr<unsigned char[]> p;
    size_t n, rb;
    Arr(size_t n_, size_t rb_, int fill) : p(new unsigned char[n_ * rb_]), n(n_), rb(rb_) { memset(p.get(), fill, n * rb); }
    template <class T>
    T *at(size_t row = 0) { return reinterpret_cast<T *>(p.get() + row * rb); }
    std::vector<unsigned char> bytes() const { return std::vector<unsigned char>(p.get(), p.get() + n * rb); }
    void set(const std::vector<unsigned char> &v) { memcpy(p.get(), v.data(), n * rb); }
    bool same_row(const std::vector<unsigned char> &v, size_t row) const { return !memcmp(p.get() + row * rb, v.data() + row * rb, rb); }
};

struct Batch {
    const int *sh;
    int R, C, k, sm, N, A, W;
    int64_t n;
    Arr board, rng, timer, eff, actions, reward, n_new, n_act, flags, term, mask, left, fin, obs;
    Batch(const int *s, int64_t n_)
        : sh(s), R(s[0]), C(s[1]), k(s[2]), sm(s[3]), N(R * C), A(2 * N - R - C), W((A + 63) / 64), n(n_),
          board(n, 2 * N, 0x5A), rng(n, 40, 0), timer(n, 4, 0x5A), eff(n, 8 * W, 0x5A), actions(n, 4, 0),
          reward(n, 4, 0x5A), n_new(n, 4, 0x5A), n_act(n, 4, 0x5A), flags(n, 1, 0x5A), term(n, 4, 0x5A),
          mask(n, A, 0x5A), left(n, 8, 0x5A), fin(n, 2 * N, 0x5A), obs(n, 8 * N, 0x5A) {}
    std::vector<Arr *> all() {
        return {&board, &rng, &timer, &eff, &actions, &reward, &n_new, &n_act, &flags, &term, &mask, &left, &fin, &obs};
    }
    std::vector<Arr *> state() { return {&board, &rng, &timer, &eff}; }
    // a normal tile of colour 1 in the first cell of every third board
    void edit() {
        for (int64_t e = 0; e < n; e += 3) { board.at<int8_t>(e)[0] = 1; board.at<int8_t>(e)[N] = 1; }
    }
    // the vector outputs as a caller initialises them after a reset
    void init_outputs() {
        for (int64_t e = 0; e < n; e++) {
            for (int a = 0; a < A; a++) mask.at<uint8_t>(e)[a] = (uint8_t)((eff.at<uint64_t>(e)[a >> 6] >> (a & 63)) & 1);
            for (int c = 0; c < 2 * N; c++) obs.at<int32_t>(e)[c] = board.at<int8_t>(e)[c];
            *left.at<int64_t>(e) = kMoves - *timer.at<int32_t>(e);
            memset(term.at<uint8_t>(e), 0, 4);
        }
    }
    // one step of rows [lo, n): every pointer and the policy's first env move with lo
    void step(int64_t lo, int trust, int mode, int policy, int32_t t) {
        emu_step(R, C, k, sm, kMoves, n - lo, board.at<int8_t>(lo), rng.at<uint64_t>(lo), timer.at<int32_t>(lo),
                 actions.at<int32_t>(lo), reward.at<int32_t>(lo), n_new.at<int32_t>(lo), n_act.at<int32_t>(lo),
                 flags.at<uint8_t>(lo), eff.at<uint64_t>(lo), trust, mode, policy, kKey, kFirst + lo, t,
                 term.at<uint8_t>(lo), mask.at<uint8_t>(lo), left.at<int64_t>(lo), fin.at<int8_t>(lo),
                 obs.at<int32_t>(lo));
    }
};

long g_cases = 0;

// T trusted, U untrusted after a hand edit, P the in-kernel policy.  The second
// step ends every episode: mode 0 then steps after done, mode 1 regenerates in
// the same call (so its U runs on fresh boards), mode 2 resets in the third.
const char *schedule(int mode) { return mode == 1 ? "TPU" : "TUP"; }

void run_steps(Batch &b, const std::vector<std::vector<unsigned char>> &start, std::mt19937_64 &g, int mode, int64_t lo) {
    const auto st = b.state();
    for (size_t i = 0; i < st.size(); i++) st[i]->set(start[i]);
    b.init_outputs();
    std::vector<std::vector<unsigned char>> before;
    const char *sched = schedule(mode);
    for (int t = 0; t < 3; t++) {
        if (sched[t] == 'U') b.edit();
        for (int64_t e = 0; e < b.n; e++) *b.actions.at<int32_t>(e) = (int32_t)(g() % (uint64_t)b.A);
        before.clear();
        for (Arr *a : b.all()) before.push_back(a->bytes());
        b.step(lo, sched[t] != 'U', mode, sched[t] == 'P', t);
        const auto all = b.all();
        for (size_t i = 0; i < all.size(); i++)
            for (int64_t e = 0; e < lo; e++)
                if (!all[i]->same_row(before[i], e)) die("a step of rows [1, n) wrote row 0", b.sh, b.n);
        for (int64_t e = lo; e < b.n; e++) {
            const int32_t tm = *b.timer.at<int32_t>(e);
            if (tm < 0 || tm > kMoves) die("timer out of range after a step", b.sh, b.n);
            if (sched[t] == 'P' && (uint32_t)*b.actions.at<int32_t>(e) >= (uint32_t)b.A) die("policy action out of range", b.sh, b.n);
        }
    }
    g_cases++;
}

void run_shape(const int *sh, int64_t n, std::mt19937_64 &g) {
    Batch b(sh, n);
    for (int64_t e = 0; e < n; e++) {                    // PCG64 words: any state, an odd increment, no buffered half
        uint64_t *w = b.rng.at<uint64_t>(e);
        w[0] = g(); w[1] = g(); w[2] = g() | 1; w[3] = g(); w[4] = 0;
    }
    emu_reset(b.R, b.C, b.k, b.sm, kMoves, n, b.board.at<int8_t>(), b.rng.at<uint64_t>(), b.timer.at<int32_t>(),
              b.eff.at<uint64_t>());
    for (int64_t e = 0; e < n; e++)
        if (*b.timer.at<int32_t>(e) != 0) die("reset left a timer", sh, n);
    g_cases++;

    // masked reset: row 0, row n - 1 and every third of the rest; the other rows keep their bytes
    {
        Arr sel(n, 1, 0);
        for (int64_t e = 0; e < n; e++) *sel.at<uint8_t>(e) = (e == 0 || e == n - 1 || e % 3 == 1) ? (uint8_t)(1 + 127 * (e & 1)) : 0;
        for (int64_t e = 0; e < n; e++) *b.timer.at<int32_t>(e) = 1;
        std::vector<std::vector<unsigned char>> before;
        for (Arr *a : b.state()) before.push_back(a->bytes());
        emu_reset_masked(b.R, b.C, b.k, b.sm, kMoves, n, b.board.at<int8_t>(), b.rng.at<uint64_t>(), b.timer.at<int32_t>(),
                         b.eff.at<uint64_t>(), sel.at<uint8_t>(), 0xFF);
        const auto st = b.state();
        for (int64_t e = 0; e < n; e++) {
            if (*sel.at<uint8_t>(e)) {
                if (*b.timer.at<int32_t>(e) != 0 || st[1]->same_row(before[1], e)) die("masked reset skipped a selected row", sh, n);
            } else {
                for (size_t i = 0; i < st.size(); i++)
                    if (!st[i]->same_row(before[i], e)) die("masked reset wrote an unselected row", sh, n);
            }
        }
        for (int64_t e = 0; e < n; e++) *b.timer.at<int32_t>(e) = 0;
        g_cases++;
    }

    std::vector<std::vector<unsigned char>> start;
    for (Arr *a : b.state()) start.push_back(a->bytes());
    for (int mode = 0; mode < 3; mode++) {
        run_steps(b, start, g, mode, 0);
        if (n >= 2) run_steps(b, start, g, mode, 1);
    }

    // peek: trusted on the boards as reset left them, untrusted after a hand edit
    {
        const auto st = b.state();
        for (size_t i = 0; i < st.size(); i++) st[i]->set(start[i]);
        for (int trust = 1; trust >= 0; trust--) {
            if (!trust) b.edit();
            Arr reward(n, 4 * b.A, 0x5A), n_new(n, 4 * b.A, 0x5A), n_act(n, 4 * b.A, 0x5A), flags(n, b.A, 0x5A);
            Arr best_action(n, 4, 0x5A), best_reward(n, 4, 0x5A);
            std::vector<std::vector<unsigned char>> before;
            for (Arr *a : st) before.push_back(a->bytes());
            emu_peek(b.R, b.C, b.k, b.sm, n, b.board.at<int8_t>(), b.rng.at<uint64_t>(), b.eff.at<uint64_t>(), trust,
                     reward.at<int32_t>(), n_new.at<int32_t>(), n_act.at<int32_t>(), flags.at<uint8_t>(),
                     best_action.at<int32_t>(), best_reward.at<int32_t>());
            for (size_t i = 0; i < st.size(); i++)
                if (st[i]->bytes() != before[i]) die("peek wrote its input", sh, n);
            for (int64_t e = 0; e < n; e++)
                if ((uint32_t)*best_action.at<int32_t>(e) >= (uint32_t)b.A) die("peek best_action out of range", sh, n);
            g_cases++;
        }
    }

    // rollout, depth 2, 2 samples: horizons 2, 1, 0 in turn
    {
        const auto st = b.state();
        for (size_t i = 0; i < st.size(); i++) st[i]->set(start[i]);
        const int S = 2;
        Arr rng(S * n, 40, 0), ret(S * n, 4 * b.A, 0x5A), plies(S * n, 4 * b.A, 0x5A), flags(S * n, b.A, 0x5A);
        Arr total(n, 4 * b.A, 0x5A), best_action(n, 4, 0x5A), best_total(n, 4, 0x5A);
        for (int64_t v = 0; v < S * n; v++) {
            uint64_t *w = rng.at<uint64_t>(v);
            w[0] = g(); w[1] = g(); w[2] = g() | 1; w[3] = g(); w[4] = 0;
        }
        for (int64_t e = 0; e < n; e++) *b.timer.at<int32_t>(e) = (int32_t)(e % 3);
        std::vector<std::vector<unsigned char>> before;
        for (Arr *a : st) before.push_back(a->bytes());
        if (emu_rollout(b.R, b.C, b.k, b.sm, kMoves, n, b.board.at<int8_t>(), rng.at<uint64_t>(), b.timer.at<int32_t>(),
                        b.eff.at<uint64_t>(), 1, 2, S, kKey, kFirst, 11, ret.at<int32_t>(), plies.at<int32_t>(),
                        flags.at<uint8_t>(), total.at<int32_t>(), best_action.at<int32_t>(), best_total.at<int32_t>()))
            die("rollout refused", sh, n);
        for (size_t i = 0; i < st.size(); i++)
            if (st[i]->bytes() != before[i]) die("rollout wrote its input", sh, n);
        for (int64_t e = 0; e < n; e++)
            for (int s = 0; s < S; s++)
                for (int a = 0; a < b.A; a++)
                    if ((uint32_t)plies.at<int32_t>(s * n + e)[a] > (uint32_t)(2 - e % 3)) die("rollout past its horizon", sh, n);
        g_cases++;
    }

    // effective: hand-edited boards into an exactly sized mask block
    {
        b.edit();
        Arr eff(n, 8 * b.W, 0x5A);
        const std::vector<unsigned char> before = b.board.bytes();
        emu_effective(b.R, b.C, b.k, b.sm, n, b.board.at<int8_t>(), eff.at<uint64_t>());
        if (b.board.bytes() != before) die("effective wrote the boards", sh, n);
        if (b.A & 63)
            for (int64_t e = 0; e < n; e++)
                if (eff.at<uint64_t>(e)[b.W - 1] >> (b.A & 63)) die("effective set a bit past A", sh, n);
        g_cases++;
    }
    if (emu_status_clear() & 1u) die("a kernel reported an internal error", sh, n);
}

}  // namespace

int main() {
    // tests/extent_cases.py EXTENT_SHAPES
    const int shapes[][4] = {{3, 5, 2, 0},   {7, 9, 5, 15}, {10, 10, 4, 0}, {10, 10, 5, 0},  {10, 10, 4, 14},
                             {2, 22, 4, 0},  {2, 22, 4, 15}, {2, 64, 4, 0}, {20, 20, 6, 15}, {9, 15, 15, 0}};
    constexpr int kShapes = (int)(sizeof shapes / sizeof shapes[0]);
    // One child process per shape, all at once: the shapes are independent, the
    // emulator's state is global, and under the sanitizers the ten of them take
    // four and a half minutes in a row.  A child reports its case count through
    // a pipe; a sanitizer report aborts it, and the parent then fails.
    pid_t pid[kShapes];
    int fd[kShapes];
    fflush(nullptr);
    for (int i = 0; i < kShapes; i++) {
        int p[2];
        if (pipe(p)) { perror("extent_asan: pipe"); return 1; }
        pid[i] = fork();
        if (pid[i] < 0) { perror("extent_asan: fork"); return 1; }
        if (pid[i] == 0) {
            close(p[0]);
            std::mt19937_64 g(1 + i);
            const bool big = shapes[i][0] * shapes[i][1] > 128;
            for (int64_t n : {(int64_t)1, (int64_t)(big ? 3 : 9)}) run_shape(shapes[i], n, g);
            if (write(p[1], &g_cases, sizeof g_cases) != (ssize_t)sizeof g_cases) exit(1);
            exit(0);
        }
        close(p[1]);
        fd[i] = p[0];
    }
    long cases = 0;
    int failed = 0;
    for (int i = 0; i < kShapes; i++) {
        long c = 0;
        int status = 0;
        const bool got = read(fd[i], &c, sizeof c) == (ssize_t)sizeof c;
        close(fd[i]);
        if (waitpid(pid[i], &status, 0) != pid[i] || !WIFEXITED(status) || WEXITSTATUS(status) != 0 || !got) {
            fprintf(stderr, "extent_asan: the run of %dx%d k%d s%d failed (wait status 0x%x)\n", shapes[i][0], shapes[i][1],
                    shapes[i][2], shapes[i][3], status);
            failed++;
        }
        cases += c;
    }
    if (failed) return 1;
    printf("extent_asan ok: %ld cases\n", cases);
    return 0;
}
