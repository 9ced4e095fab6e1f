"""CPU: datasets._ReadAhead, the two staging slots and the one background reader every dataset relies on.  ``torch.cuda.Event`` is
replaced by a stub that logs ``record`` / ``synchronize``; the slots are dicts, ``read`` writes the index into its slot.  One log holds,
in the order they happen: ("prepare" | "read", thread name, index, slot id), ("record" | "sync", event number) and what the caller adds
after its own calls, ("acquired" | "released", index, slot id)."""
import threading

import pytest
import torch

N = 5
NAME = "ra-test"


class _Harness:
    def __init__(self, monkeypatch, fail_at=None, prepare=True):
        from patchrefinerv2_amd.datasets import _ReadAhead
        self.log = log = []

        class Event:
            count = 0

            def __init__(self):
                Event.count += 1
                self.k = Event.count

            def record(self):
                log.append(("record", self.k))

            def synchronize(self):
                log.append(("sync", self.k))
        monkeypatch.setattr(torch.cuda, "Event", Event)

        def read(idx, slot):
            log.append(("read", threading.current_thread().name, idx, id(slot)))
            if idx == fail_at:
                raise ValueError(f"item {idx}: broken file")
            slot["item"] = idx

        def prep(idx, slot):
            log.append(("prepare", threading.current_thread().name, idx, id(slot)))
        self.ra = _ReadAhead(N, lambda: dict(item=None), read, prep if prepare else None, name=NAME)
        self.slots = [id(s) for s in self.ra._slots]

    def get(self, idx):
        """what a dataset's __getitem__ does: acquire, take the item out of the slot, release -> the item"""
        slot = self.ra.acquire(idx)
        item = slot["item"]
        self.log.append(("acquired", idx, id(slot)))
        self.ra.release(idx)
        self.log.append(("released", idx, id(slot)))
        return item

    def reads(self):
        return [e[1:] for e in self.log if e[0] == "read"]


@pytest.fixture
def harness(monkeypatch):
    made = []

    def make(**kw):
        made.append(_Harness(monkeypatch, **kw))
        return made[-1]
    yield make
    for h in made:
        h.ra.close()


def _on_pool(thread_name):
    return thread_name.startswith(NAME)


def test_sequential_access_reads_one_ahead_on_the_pool_thread(harness):
    h = harness()
    me = threading.current_thread().name
    assert [h.get(i) for i in range(N)] == list(range(N))
    reads = h.reads()
    assert [r[1] for r in reads] == list(range(N))  # every item once, index 5 never
    assert reads[0][0] == me and all(_on_pool(r[0]) for r in reads[1:])
    assert [r[2] for r in reads] == [h.slots[i % 2] for i in range(N)]  # the slots alternate
    for i in range(1, N):  # item i is read after item i - 1 was handed out and before item i is: one ahead, not more
        at = h.log.index(("read", reads[i][0], i, reads[i][2]))
        assert h.log.index(("acquired", i - 1, h.slots[(i - 1) % 2])) < at < h.log.index(("acquired", i, h.slots[i % 2]))


def test_the_guess_follows_the_step(harness):
    h = harness()
    me = threading.current_thread().name
    assert [h.get(i) for i in (0, 2, 4)] == [0, 2, 4]
    # after one access the step is not known yet: the first guess is the next index, and item 2 is then read on the caller's thread
    # into the slot item 0 has left; from the second access on the guess follows the step (4 after 2), and nothing past the end is read
    assert [(r[1], _on_pool(r[0])) for r in h.reads()] == [(0, False), (1, True), (2, False), (4, True)]
    assert [r[2] for r in h.reads()] == [h.slots[0], h.slots[1], h.slots[0], h.slots[1]]
    assert h.reads()[2][0] == me


def test_a_wrong_guess_is_read_by_the_caller_into_the_other_slot(harness):
    h = harness()
    me = threading.current_thread().name
    assert h.get(0) == 0 and h.get(3) == 3
    reads = h.reads()
    assert [(r[0] == me, r[1]) for r in reads[:3]] == [(True, 0), (False, 1), (True, 3)]
    assert reads[1][2] == h.slots[1] and reads[2][2] == h.slots[0]  # not the slot the wrong guess went to
    assert ("acquired", 3, h.slots[0]) in h.log


def test_a_failed_read_raises_from_acquire(harness):
    h = harness(fail_at=1)
    assert h.get(0) == 0  # (release(0) started the read of item 1 on the pool thread: nothing is raised here)
    with pytest.raises(ValueError, match="item 1: broken file"):
        h.ra.acquire(1)
    assert [(_on_pool(r[0]), r[1]) for r in h.reads()] == [(False, 0), (True, 1)]


def test_prepare_runs_on_the_callers_thread_before_every_read(harness):
    h = harness()
    me = threading.current_thread().name
    for i in (0, 1, 2, 0, 4):  # in order, back, and a wrong guess
        assert h.get(i) == i
    preps = [e for e in h.log if e[0] == "prepare"]
    assert preps and all(e[1] == me for e in preps)
    seq = [e for e in h.log if e[0] in ("prepare", "read")]  # one per read, right before it, same item, same slot
    assert [e[0] for e in seq] == ["prepare", "read"] * (len(seq) // 2) and all(a[2:] == b[2:] for a, b in zip(seq[::2], seq[1::2]))
    # without a prepare callback nothing else changes
    plain = harness(prepare=False)
    assert [plain.get(i) for i in range(N)] == list(range(N)) and not [e for e in plain.log if e[0] == "prepare"]


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4), (0, 2, 4), (0, 3, 1, 2), (4, 0, 1)])
def test_a_slot_is_refilled_only_after_its_event_was_synchronised(harness, order):
    h = harness()
    assert [h.get(i) for i in order] == list(order)
    h.ra.close()  # (the read that is one ahead has finished: the log is complete)
    records = [e[1] for e in h.log if e[0] == "record"]
    released = [e[2] for e in h.log if e[0] == "released"]
    assert len(records) == len(released) == len(order)  # one event per release: the k-th event guards the k-th released slot
    guard = {}  # slot id -> (the event recorded at its last release, that record's place in the log)
    refills = 0
    for at, e in enumerate(h.log):
        if e[0] == "record":
            guard[released[records.index(e[1])]] = (e[1], at)
        elif e[0] == "read" and e[3] in guard:
            event, since = guard[e[3]]
            assert ("sync", event) in h.log[since:at], (order, e)
            refills += 1
    assert refills >= len(order) - 2  # (the check above ran: only a slot's first use can come before any release of it)


def test_close_waits_for_the_pending_read(harness):
    h = harness()
    assert h.get(0) == 0
    fut = h.ra._pending[2]
    h.ra.close()
    assert fut.done() and h.ra._pending is None and [r[1] for r in h.reads()] == [0, 1]
