"""CPU: the overlap-blend pass walker of the frame driver (frame.FrameDriver._blend_passes), driven with a recording stand-in for the
running-average map -- the steps it takes for every pass structure, for a [H, W] map, for B maps and for the patch-sharded mode's
per-gather-group calls."""
import pytest
import torch

from patchrefinerv2_amd import frame
from patchrefinerv2_amd import models as M

PH, PW, RH, RW, RAW = 4, 6, 8, 12, (32, 48)
TILE_CFG = dict(patch_raw_shape=(RH, RW), image_raw_shape=list(RAW))
FIXED = [("init", 16), ("grid", 12), ("grid", 12), ("grid", 9)]
FIXED_STEPS = [("paste", 16, 4, 6), ("update", 12, 4, 6), ("update", 12, 4, 6), ("update", 9, 4, 6)]
#        passes                      expected steps                                                gather groups (pass indices)
CASES = [([("init", 16)],            [("paste", 16, 4, 6)],                                        [[0]]),
         (FIXED,                     FIXED_STEPS,                                                  [[0, 1, 2, 3]]),
         (FIXED + [("random", 32)],  FIXED_STEPS + [("resize", 32, 48), ("update", 32, 8, 12)],    [[0, 1, 2, 3], [4]]),
         (FIXED + [("random", 0)],   FIXED_STEPS + [("resize", 32, 48)],                           [[0, 1, 2, 3]])]


class _Host(M._PatchModel):
    def __init__(self):
        super().__init__()
        self.patch_process_shape = (PH, PW)

    def _pack(self):
        pass


class _RecordingMap:
    """what the walker may call on a DeviceRunningAverageMap; logs the steps, does no arithmetic"""

    def __init__(self):
        self.steps, self.shapes, self.masks = [], [], []

    def _tiles(self, step, preds, mask, tiles, th, tw):
        self.steps.append((step, preds.shape[-3], th, tw))
        self.shapes.append((tuple(preds.shape), tuple(tiles.shape)))
        self.masks.append(mask)

    def paste(self, preds, mask, tiles, th, tw):
        self._tiles("paste", preds, mask, tiles, th, tw)

    def update(self, preds, mask, tiles, th, tw):
        self._tiles("update", preds, mask, tiles, th, tw)

    def resize(self, resolution):
        self.steps.append(("resize", int(resolution[0]), int(resolution[1])))


@pytest.fixture
def host(monkeypatch):
    monkeypatch.setattr(frame, "blend_mask", lambda size, border, add, device: (tuple(size), border, add))  # (no Gaussian of a 4 x 6 box)
    return _Host()


@pytest.mark.parametrize("lead", [(), (3,)], ids=["map_2d", "map_3d_B3"])
def test_pass_walker_steps_and_tile_axis_slices(host, lead):
    for passes, steps, _ in CASES:
        n = sum(k for _, k in passes)
        ram = _RecordingMap()
        host._blend_passes(ram, passes, torch.zeros(lead + (n, PH, PW)), torch.zeros(lead + (n, 2), dtype=torch.int32), TILE_CFG)
        assert ram.steps == steps
        tiled = [s for s in steps if s[0] != "resize"]
        assert ram.shapes == [(lead + (k, PH, PW), lead + (k, 2)) for _, k, _, _ in tiled]
        assert ram.masks == [((RH, RW), host.blend_border, 1e-3) if th == RH else ((PH, PW), host.blend_border, 0.0) for _, _, th, _ in tiled]


def test_pass_walker_per_gather_group_equals_unsharded(host):
    """the patch-sharded driver's calls: one per gather group with the group's passes and its slice of the tile axis; the empty random
    pass (in no group: nothing to compute) goes along with the last group"""
    for passes, steps, group_ids in CASES:
        plan = dict(kinds=[kind for kind, _ in passes], counts=[k for _, k in passes])
        groups = host.shard_layout(plan["kinds"], plan["counts"], 2, 0)
        assert [g["passes"] for g in groups] == group_ids
        n = sum(plan["counts"])
        preds, proc = torch.zeros(n, PH, PW), torch.zeros((n, 2), dtype=torch.int32)
        ram = _RecordingMap()
        for gi, g in enumerate(groups):
            lo, hi = g["base"], g["base"] + g["n"]
            host._blend_passes(ram, host._group_passes(plan, groups, gi), preds[lo:hi], proc[lo:hi], TILE_CFG)
        assert ram.steps == steps
