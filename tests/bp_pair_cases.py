"""Cases for the paired redraw loop of bp_generate (csrc/tmg_board.hip,
bp_redraw_pairs): generate_board's redraws traced with the oracle's own
primitives, the guess rule restated on that trace, and the streams the tests
pick from it."""
import numpy as np

# (R, C, k): what each shape is there for
PAIR_SHAPES = [
    (10, 10, 4),        # the flagship shape
    (10, 10, 5),        # Lemire rejections
    (4, 4, 3),          # R < 5: guesses below row 0 and past the last row; shuffles while generating
    (3, 28, 6),         # R < 4: nearly every guess is a duplicate of the last row
    (16, 8, 4),         # the last lane of a 16-lane group holds a row
    (5, 6, 7),          # three planes
]
OLD_LOOP_SHAPE = (17, 7, 4)     # R > 16: outside bp_pair_shape, the one-redraw loop


def trace_generate(orc, R, C, k, words, max_redraws=100000):
    """generate_board's remove_colour_lines (board.py:95-131) up to its first
    line-free board: ([row count rho of each redraw], colours drawn, board,
    rng).  No shuffle is followed: the caller compares board and rng with
    orc.generate where it needs the trace validated (they agree whenever the
    first line-free board has a possible move)."""
    rng = np.array(words, dtype=np.uint64).copy()
    cols, rng = orc.rng_colours(rng, k, R * C)
    b = np.ones((2, R, C), np.int8)
    b[0] = cols.reshape(R, C)
    rows, drawn = [], R * C
    while len(rows) < max_redraws:
        lines = orc.get_colour_lines(b, k, 0)
        if not lines:
            break
        row = min(R - 1, lines[0][0][0] + 1)
        cols, rng = orc.rng_colours(rng, k, (row + 1) * C)
        b[0, :row + 1] = cols.reshape(row + 1, C)
        rows.append(row)
        drawn += (row + 1) * C
    return rows, drawn, b, rng


def pair_rounds(rows):
    """bp_redraw_pairs' bookkeeping on a traced board: (rounds, second redraws
    accepted, second redraws rejected).  A round applies redraw i and guesses
    the next row count as rows[i] - 1, rows[i] or rows[i] + 1."""
    i = rounds = acc = rej = 0
    while i < len(rows):
        rounds += 1
        if i + 1 >= len(rows):
            break                                     # the round's search found no line: neither
        if abs(rows[i + 1] - rows[i]) <= 1:
            acc += 1
            i += 2
        else:
            rej += 1
            i += 1
    return rounds, acc, rej


def long_board_seed(orc, R, C, k, seeds, more_than):
    """The first seed of `seeds` whose board takes more than `more_than` redraws."""
    from tile_match_gym_amd.seeding import batch_rng_words
    w = batch_rng_words(seeds)
    for i, s in enumerate(seeds):
        if len(trace_generate(orc, R, C, k, w[i])[0]) > more_than:
            return s
    raise AssertionError(f"no board of more than {more_than} redraws among {len(seeds)} seeds")


def second_redraws(rows):
    """Indices (into rows) of the redraws bp_redraw_pairs takes as a round's accepted second redraw."""
    out, i = set(), 0
    while i + 1 < len(rows):
        if abs(rows[i + 1] - rows[i]) <= 1:
            out.add(i + 1)
            i += 2
        else:
            i += 1
    return out


def rejection_cases(orc, R, C, k, n=4, first_seed=4000, seeds=64):
    """Streams with one Lemire-rejected word placed with the oracle's trace:
    (inside, beyond), each (words (n, 5), positions).  inside: the rejected
    draw is a colour of an accepted second redraw (every draw before it is
    accepted, so up to there draw index = colour index and the trace is the
    kernel's).  beyond: it is the first draw after the board's last colour.
    Half of each with a buffered half-word (draw 0)."""
    from rejection_states import words_rejecting_at
    from tile_match_gym_amd.seeding import batch_rng_words
    N = R * C
    base = batch_rng_words(range(first_seed, first_seed + seeds))
    inside, beyond = [], []
    for i in range(seeds):
        for want, step in ((inside, 7), (beyond, C)):
            buffered = len(want) % 2 == 1
            if len(want) >= n:
                continue
            for d in range(N + step, N + 1500, step):
                w = words_rejecting_at(base[i:i + 1], d, buffered=buffered)[0]
                rows, drawn, _, _ = trace_generate(orc, R, C, k, w)
                if want is beyond:
                    hit = drawn == d
                else:
                    hit, start = False, N
                    for j, row in enumerate(rows):
                        if start <= d < start + (row + 1) * C:
                            hit = j in second_redraws(rows)
                            break
                        start += (row + 1) * C
                if hit:
                    want.append((w, d))
                    break
        if len(inside) >= n and len(beyond) >= n:
            break
    assert len(inside) >= n and len(beyond) >= n, (len(inside), len(beyond))
    return tuple((np.stack([w for w, _ in c]), np.array([d for _, d in c])) for c in (inside, beyond))
