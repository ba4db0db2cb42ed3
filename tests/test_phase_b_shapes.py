"""The scenes of tests/phase_b_shapes.py reach what the phase B tests need, judged by the C oracle's labels of sweep 1
under the host's layout (util.entry_layout): every matrix row, a one-pose last chunk, both sides of the CH boundaries,
chunks with exactly 224 / 225 and superchunks with exactly 1536 / 1537 distinct labels, fresh landmarks beyond chunk
512."""
import os

import numpy as np
import pytest

import phase_b_shapes as pb
from util import entry_layout


@pytest.fixture(autouse=True, scope="module")
def _threads():
    from oracle import c_oracle as co
    co.set_threads(min(16, int(os.environ.get("OMP_NUM_THREADS", "8") or 8)))


def test_layout_mirror_at_the_edges():
    assert entry_layout(16383)["chunk_poses"] == 16 and entry_layout(16384)["chunk_poses"] == 32
    assert entry_layout(65535)["chunk_poses"] == 32 and entry_layout(65536)["chunk_poses"] == 64
    for n in (1, 15, 16, 17, 1023, 1024, 1025, 4096, 16383, 16384, 40001, 65535, 65536, 70000, 200000):
        lay = entry_layout(n)
        CH, G, ns, nc = lay["chunk_poses"], lay["chunk_group"], lay["nsuper"], lay["nchunks"]
        assert (nc - 1) * CH < n <= nc * CH and ns <= 64 and (ns - 1) * G < nc <= ns * G
        assert G == 1 or (G - 1) * 64 < nc


EXPECT = {   # scene: (CH, G, nsuper, poses in the last chunk, chunks in the last superchunk)
    "layout:1024": (16, 1, 64, 16, 1),
    "layout:4096": (16, 4, 64, 16, 4),
    "layout:1025": (16, 2, 33, 1, 1),
    "layout:16383": (16, 16, 64, 15, 16),
    "layout:16384": (32, 8, 64, 32, 8),
    "layout:40001": (32, 20, 63, 1, 11),
    "layout:65535": (32, 32, 64, 31, 32),
    "layout:65536": (64, 16, 64, 64, 16),
}


@pytest.mark.parametrize("name", pb.LAYOUT)
def test_layout_scenes_reach_their_layout(name):
    sc = pb.scene(name)
    r = pb.reach(sc)
    lay = r["layout"]
    CH, G, ns, last_poses, last_chunks = EXPECT[name]
    assert (lay["chunk_poses"], lay["chunk_group"], lay["nsuper"]) == (CH, G, ns)
    assert r["last_chunk_poses"] == last_poses and lay["nchunks"] - (ns - 1) * G == last_chunks
    # every matrix row holds labels (the last one included), every chunk too
    assert (r["per_super"] > 0).all() and (r["per_chunk"] > 0).all()
    assert r["entries"][-1] > 0
    assert pb.expected_path(r) == "hier"
    assert np.abs(sc.x_true[:2]).max() < 50.0, "coordinates stay small: target errors are judged in metres"
    print("%s: CH %d G %d nsuper %d, entries per pose <= %d, labels per chunk <= %d, per superchunk <= %d"
          % (name, CH, G, ns, r["entries"].max(), r["per_chunk"].max(), r["per_super"].max()))


@pytest.mark.parametrize("name", pb.LIMITS)
def test_limit_scenes_reach_exact_counts(name):
    sc = pb.scene(name)
    r = pb.reach(sc)
    kind = name.split(":")[0]
    target = int(kind[5:])
    assert r["entries"].max() <= pb.WAVE
    if kind.startswith("chunk"):
        assert r["per_chunk"].max() == target and np.sort(r["per_chunk"])[-2] <= pb.CHUNK_CAP
        assert r["per_super"].max() <= pb.SUPER_CAP
    else:
        assert r["layout"]["chunk_group"] >= 7
        assert r["per_super"].max() == target and np.sort(r["per_super"])[-2] <= pb.SUPER_CAP
        assert r["per_chunk"].max() <= pb.CHUNK_CAP
    assert pb.expected_path(r) == ("hier" if target in (224, 1536) else "sort")
    print("%s: CH %d G %d, entries per pose <= %d, labels per chunk <= %d, per superchunk <= %d, clutter poses %d"
          % (name, r["layout"]["chunk_poses"], r["layout"]["chunk_group"], r["entries"].max(), r["per_chunk"].max(),
             r["per_super"].max(), sc.clutter.size))


def test_limit_scenes_cover_both_chunk_sizes():
    assert {entry_layout(int(n.split(":")[1]))["chunk_poses"] for n in pb.LIMITS if n.startswith("chunk")} == {16, 32}


def test_ranks_scene_creates_landmarks_beyond_chunk_512():
    sc = pb.scene("ranks")
    r = pb.reach(sc)
    lay = r["layout"]
    assert lay["nchunks"] > 512 and pb.expected_path(r) == "hier"
    cc = set(r["creator_chunks"].tolist())
    assert 0 in cc and lay["nchunks"] - 1 in cc and len([c for c in cc if c > 512]) >= 4
    assert set(r["creators"].tolist()) == set(sc.clutter.tolist()), "exactly the clutter poses create landmarks"
