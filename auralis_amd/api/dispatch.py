"""ChunkPlacer — which engine runs which chunk when one process drives several engines (one per GPU; SURVEY §7 "host dispatcher").

Late binding.  Phase 1 hands over every chunk of a request at once (a book is ~500 of them) and a chunk's length is unknown until
its stop token (4 to 605 tokens), so dealing them out on arrival by "least loaded" would count chunks, not work, and degenerate to
round-robin.  The placer therefore keeps the chunks in ONE queue of its own and gives an engine a chunk only while that engine's
outstanding sequences (placed here and not yet resolved) are below

    backlog(e) = max_seqs(e) + max(1, max_seqs(e) // 8)

-- its slots plus one default `admit_min_batch` group, so the engine's grouped admission still finds a group to take -- and tops the
engine up from the queue whenever one of its sequences resolves (finished, failed or cancelled).  Work is thus pulled by the engines
that finish theirs, which is list scheduling: the makespan stays within Graham's bound of the optimum plus what the per-engine backlog
can strand on one engine at the very end (tests/test_dispatch.py simulates it).

Among engines with room the one with the fewest outstanding sequences gets the chunk; ties go to the lower `token_budget`
(aur_get_load), then to the lower index.  An urgent chunk (`priority > 0`: the head of a stream somebody is waiting to hear) is never
queued: it overtakes everything and goes, backlog or not, to the engine with the fewest RUNNING sequences, where the engine's own
`urgent_rows` logic then acts.

The class is deliberately inert: no threads, no asyncio, no clocks.  Its caller serialises the calls (XTTSv2Engine holds one lock
around them) and performs the submission inside the `place` callback, so a lock-step simulation can drive it as well."""
from __future__ import annotations

import collections
from typing import Any, Callable, List, Optional, Sequence


class EngineUnavailable(RuntimeError):
    """Raised by a `place` callback: this engine takes no more work (its driver has stopped).  Also raised by `submit` when no engine
    is left."""


def backlog(max_seqs: int) -> int:
    return int(max_seqs) + max(1, int(max_seqs) // 8)


class ChunkPlacer:
    def __init__(self, max_seqs: Sequence[int], place: Callable[[int, Any], Optional[bool]],
                 budget: Optional[Callable[[int], int]] = None, running: Optional[Callable[[int], int]] = None):
        """`max_seqs[e]`: slots of engine e.  `place(e, item)`: submit `item` to engine e now; returning False means the item is
        spent without occupying the engine (its submission failed for a reason of its own, the callback has told its owner);
        raising EngineUnavailable means engine e is gone and the item is still to be placed.  `budget(e)` / `running(e)`: the
        engine's aur_load.token_budget / .running at this moment (asked only to break ties / to place an urgent chunk)."""
        self.backlog = [backlog(s) for s in max_seqs]
        self.outstanding = [0] * len(self.backlog)
        self.alive = [True] * len(self.backlog)
        self.placed_total = [0] * len(self.backlog)
        self._place = place
        self._budget = budget or (lambda e: 0)
        self._running = running or (lambda e: self.outstanding[e])
        self._queue: "collections.deque" = collections.deque()

    # ------------------------------------------------------------------ queries
    def queued(self) -> int:
        return len(self._queue)

    def engines_alive(self) -> List[int]:
        return [e for e, a in enumerate(self.alive) if a]

    # ------------------------------------------------------------------ events
    def submit(self, item: Any, priority: int = 0) -> None:
        if not any(self.alive):
            raise EngineUnavailable("no engine left: every engine driver has stopped")
        if priority > 0:
            self._place_urgent(item)
        else:
            self._queue.append(item)
            self._pump()

    def resolved(self, e: int) -> None:
        """One sequence placed on engine e has resolved (finished, failed or cancelled)."""
        if self.outstanding[e] > 0:
            self.outstanding[e] -= 1
        self._pump()

    def cancel(self, item: Any) -> bool:
        """Remove `item` if it is still queued here (no engine has seen it).  False: it was placed (or is unknown)."""
        try:
            self._queue.remove(item)
            return True
        except ValueError:
            return False

    def engine_dead(self, e: int) -> List[Any]:
        """Engine e takes no more work.  What was queued goes to the others; returns the items nobody can take any more (all of the
        queue once the last engine is gone, else nothing)."""
        self.alive[e] = False
        self._pump()
        return self.orphans()

    def orphans(self) -> List[Any]:
        """Once no engine is left (the last one may have been found gone inside a `place`): the queue, emptied.  Else nothing."""
        if any(self.alive):
            return []
        out = list(self._queue)
        self._queue.clear()
        return out

    # ------------------------------------------------------------------ placement
    def _pick(self) -> int:
        cands = [e for e in range(len(self.backlog)) if self.alive[e] and self.outstanding[e] < self.backlog[e]]
        if not cands:
            return -1
        least = min(self.outstanding[e] for e in cands)
        cands = [e for e in cands if self.outstanding[e] == least]
        if len(cands) == 1:
            return cands[0]
        return min(cands, key=lambda e: (self._budget(e), e))

    def _hand(self, e: int, item: Any) -> bool:
        """True: the item is off our hands (placed or spent); False: engine e turned out to be gone."""
        try:
            took = self._place(e, item)
        except EngineUnavailable:
            self.alive[e] = False
            return False
        if took is not False:
            self.outstanding[e] += 1
            self.placed_total[e] += 1
        return True

    def _pump(self) -> None:
        while self._queue:
            e = self._pick()
            if e < 0:
                return
            if self._hand(e, self._queue[0]):
                self._queue.popleft()

    def _place_urgent(self, item: Any) -> None:
        while True:
            cands = self.engines_alive()
            if not cands:
                raise EngineUnavailable("no engine left: every engine driver has stopped")
            e = min(cands, key=lambda i: (self._running(i), self.outstanding[i], self._budget(i), i))
            if self._hand(e, item):
                return
