"""CPU: ChunkPlacer (auralis_amd/api/dispatch.py) alone -- the placement rules one by one, then a lock-step simulation of a book on
eight engines against the list-scheduling lower bound and against static dealing (parallel.shard_units)."""
import collections
import heapq
import math
import random

import pytest

from auralis_amd.api.dispatch import ChunkPlacer, EngineUnavailable, backlog


class Log:
    """place callback that records (engine, item) and keeps the tables a test sets for budget / running"""

    def __init__(self, n):
        self.placed = []
        self.budget = [0] * n
        self.running = [0] * n
        self.gone = set()

    def place(self, e, item):
        if e in self.gone:
            raise EngineUnavailable(str(e))
        self.placed.append((e, item))

    def placer(self, max_seqs):
        return ChunkPlacer(max_seqs, self.place, budget=lambda e: self.budget[e], running=lambda e: self.running[e])


def test_backlog_is_slots_plus_one_default_admission_group():
    assert [backlog(s) for s in (1, 4, 8, 64, 192)] == [2, 5, 9, 72, 216]


def test_backlog_bound_holds_and_resolutions_top_up():
    log = Log(2)
    p = log.placer([4, 4])
    for i in range(30):
        p.submit(i)
        assert all(o <= 5 for o in p.outstanding)
    assert p.outstanding == [5, 5] and p.queued() == 20 and [i for _, i in log.placed] == list(range(10))   # FIFO
    p.resolved(1)
    assert log.placed[-1] == (1, 10) and p.outstanding == [5, 5] and p.queued() == 19
    for _ in range(3):
        p.resolved(0)
    assert [x for x in log.placed[-3:]] == [(0, 11), (0, 12), (0, 13)] and max(p.outstanding) == 5


def test_tie_breaks_outstanding_then_budget_then_index():
    log = Log(3)
    p = log.placer([4, 4, 4])
    log.budget = [10, 5, 5]
    p.submit("a")                      # all at 0 outstanding: lower budget, then lower index -> 1
    p.submit("b")                      # 0 and 2 at 0: budget 10 vs 5 -> 2
    p.submit("c")                      # only 0 has none outstanding: fewest outstanding beats its budget
    assert log.placed == [(1, "a"), (2, "b"), (0, "c")]
    log.budget = [7, 7, 7]
    p.submit("d")
    assert log.placed[-1] == (0, "d")  # all equal: lower index


def test_urgent_overtakes_the_queue_and_goes_to_the_fewest_running():
    log = Log(2)
    p = log.placer([4, 4])
    for i in range(14):
        p.submit(i)
    assert p.outstanding == [5, 5] and p.queued() == 4
    log.running = [4, 2]
    p.submit("urgent", priority=1)
    assert log.placed[-1] == (1, "urgent") and p.outstanding == [5, 6] and p.queued() == 4   # past its backlog, queue untouched
    p.resolved(1)                      # 1 is AT its backlog now: nothing is topped up
    assert p.outstanding == [5, 5] and p.queued() == 4
    p.resolved(1)
    assert log.placed[-1] == (1, 10)


def test_a_queued_chunk_is_cancelled_without_any_engine_seeing_it():
    log = Log(2)
    p = log.placer([1, 1])
    for i in range(6):
        p.submit(i)
    assert p.queued() == 2 and p.cancel(4) and not p.cancel(4) and not p.cancel(0)   # 0 was placed: the caller tells its engine
    for _ in range(4):
        p.resolved(0)
    assert [i for _, i in log.placed] == [0, 1, 2, 3, 5]


def test_a_dead_engines_unplaced_share_goes_to_the_others():
    log = Log(3)
    p = log.placer([2, 2, 2])
    for i in range(20):
        p.submit(i)
    n0 = len(log.placed)
    assert n0 == 9 and p.engine_dead(0) == []
    for _ in range(40):
        p.resolved(1)
        p.resolved(2)
    assert sorted(i for _, i in log.placed) == list(range(20))
    assert all(e != 0 for e, _ in log.placed[n0:])
    # an engine found gone inside place(): the chunk is still placed, elsewhere, once
    log.gone.add(1)
    p.submit("x")
    assert log.placed[-1] == (2, "x") and p.engines_alive() == [2]
    # the last engine goes: what is queued comes back to the caller, and nothing more is accepted
    for i in range(5):
        p.submit(("q", i))
    left = p.queued()
    assert left > 0 and len(p.engine_dead(2)) == left and p.queued() == 0
    with pytest.raises(EngineUnavailable):
        p.submit("y")
    with pytest.raises(EngineUnavailable):
        p.submit("z", priority=1)


def test_a_chunk_that_fails_on_its_own_does_not_occupy_the_engine():
    placed = []
    p = ChunkPlacer([2], lambda e, item: placed.append(item) or (item != "bad"))
    p.submit("bad")
    p.submit("ok")
    assert placed == ["bad", "ok"] and p.outstanding == [1]


def test_every_chunk_is_placed_exactly_once_under_random_events():
    rng = random.Random(7)
    log = Log(4)
    p = log.placer([3, 2, 4, 1])
    submitted, cancelled = [], set()
    for step in range(4000):
        r = rng.random()
        if r < 0.45:
            submitted.append(step)
            p.submit(step, priority=1 if rng.random() < 0.05 else 0)
        elif r < 0.9:
            e = rng.randrange(4)
            if p.outstanding[e]:
                p.resolved(e)
        elif submitted:
            c = rng.choice(submitted)
            if p.cancel(c):
                cancelled.add(c)
        assert all(p.outstanding[e] <= p.backlog[e] + 40 for e in range(4))
    while p.queued():
        for e in range(4):
            if p.outstanding[e]:
                p.resolved(e)
    got = [i for _, i in log.placed]
    assert len(got) == len(set(got)) and set(got) == set(submitted) - cancelled
    assert sum(p.placed_total) == len(got)


# ------------------------------------------------------------------------------------------------ lock-step simulation
N_ENGINES, SLOTS, LONGEST = 8, 4, 605


def book(seed):
    """Chunk lengths in tokens: 4..605, mean ~219 (the c5s.tokens_per_chunk range and mean of BENCH_r06.json), enough of them that
    total / (N * S) >= 40 * 605."""
    rng = random.Random(seed)
    out, total = [], 0
    while total < 40 * LONGEST * N_ENGINES * SLOTS:
        out.append(4 + int(round(601 * rng.betavariate(1.2, 2.15))))
        total += out[-1]
    return out


def makespan_placer(lengths):
    """One tick: every engine seats what waits into its free slots, then every running sequence makes one token; a sequence that
    made its last one resolves (the placer tops its engine up; the newcomer is seated in the next tick at the earliest... or in this
    one, on an engine whose turn has not come yet)."""
    waiting = [collections.deque() for _ in range(N_ENGINES)]
    running = [[] for _ in range(N_ENGINES)]
    worst = [0]

    def place(e, i):
        waiting[e].append(lengths[i])
        worst[0] = max(worst[0], len(waiting[e]) + len(running[e]))

    p = ChunkPlacer([SLOTS] * N_ENGINES, place, budget=lambda e: sum(waiting[e]) + sum(running[e]), running=lambda e: len(running[e]))
    for i in range(len(lengths)):
        p.submit(i)
    ticks = 0
    while p.queued() or any(waiting[e] or running[e] for e in range(N_ENGINES)):
        ticks += 1
        for e in range(N_ENGINES):
            while waiting[e] and len(running[e]) < SLOTS:
                running[e].append(waiting[e].popleft())
            left = [r - 1 for r in running[e]]
            running[e] = [r for r in left if r > 0]
            for _ in range(len(left) - len(running[e])):
                p.resolved(e)
    assert worst[0] <= backlog(SLOTS)
    assert sum(p.placed_total) == len(lengths)
    return ticks


def makespan_static(lengths):
    """parallel.shard_units dealing in blocks of 8 (longform.stream_sharded's default paragraphs_per_block is what the torchrun path
    uses); every engine works through its share in order on its S slots."""
    from auralis_amd.parallel import shard_units
    worst = 0
    for r in range(N_ENGINES):
        slots = [0] * SLOTS
        heapq.heapify(slots)
        for i in shard_units(len(lengths), N_ENGINES, r, per_gpu_batch=8):
            heapq.heappush(slots, heapq.heappop(slots) + lengths[i])
        worst = max(worst, max(slots))
    return worst


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_simulated_book_on_eight_engines(seed):
    lengths = book(seed)
    total = sum(lengths)
    assert min(lengths) >= 4 and max(lengths) <= LONGEST and 200 <= total / len(lengths) <= 240
    assert total / (N_ENGINES * SLOTS) >= 40 * LONGEST
    lb = max(LONGEST, math.ceil(total / (N_ENGINES * SLOTS)))
    placed, static = makespan_placer(lengths), makespan_static(lengths)
    print(f"seed {seed}: {len(lengths)} chunks, {total} tokens, LB {lb}: placer {placed} = {placed / lb:.4f} LB, "
          f"static dealing {static} = {static / lb:.4f} LB")
    assert placed <= 1.05 * lb
    assert placed <= static
