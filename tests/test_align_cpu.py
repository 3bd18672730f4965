"""align_trajectories without a GPU: the local alignment of deep_cartograph_amd/sequence.py against the pure-Python
oracle (tests/align_oracle.py) on inputs whose optimum the oracle finds unique, the documented tie rule on an input
whose optimum is not, sequences and residue maps of edited copies of the fixture topology, the C-alpha fit selection,
and the tool's refusals.  The fixture is the trajectory and topology of tests/golden/compute_features_golden.npz."""
import dataclasses

import numpy as np
import pytest

from deep_cartograph_amd import _lib, sequence, trajectory
from tests import align_oracle as ao
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def fixture_files(tmp_path_factory):
    g = load_golden("compute_features_golden.npz")
    d = tmp_path_factory.mktemp("align_cpu")
    dcd, pdb = str(d / "CA_example.dcd"), str(d / "CA_example.pdb")
    with open(dcd, "wb") as f:
        f.write(g["dcd"].tobytes())
    with open(pdb, "w") as f:
        f.write(str(g["pdb"]))
    return dcd, pdb


@pytest.fixture(scope="module")
def top(fixture_files):
    return trajectory.read_topology(fixture_files[1])


@pytest.fixture(scope="module")
def seq(top):
    return sequence.residue_sequence(top)[0]


def edited(top, keep=None, shift=0):
    """A copy of a topology with the atoms `keep` (default all) and the resids shifted."""
    keep = np.arange(top.n_atoms) if keep is None else np.asarray(keep)
    return trajectory.Topology([top.names[i] for i in keep], [top.resnames[i] for i in keep], [top.chains[i] for i in keep],
                               [top.segids[i] for i in keep], top.resids[keep] + shift, top.positions[keep].copy(), None)


def appended(top, name, resname, chain, resid):
    return trajectory.Topology(top.names + [name], top.resnames + [resname], top.chains + [chain], top.segids + [chain],
                               np.append(top.resids, resid), np.vstack([top.positions, [[1.0, 2.0, 3.0]]]).astype(np.float32), None)


def mutate(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "A" if s[p] == "W" else "W"
    return "".join(s)


def test_fixture_sequence(top, seq):
    letters, resids = sequence.residue_sequence(top)
    assert len(letters) == 104 and letters.startswith("QSPYSAAMAE")
    assert resids == list(range(504, 608)) and set(top.chains) == {"B"}


def cases(seq):
    mut = mutate(seq, (20, 21, 70))
    out = [("identical", seq, 104.0, 104), ("ends removed", seq[5:-3], 96.0, 96)]
    out += [(f"deleted [{lo},{lo + 7})", seq[:lo] + seq[lo + 7:], 92.0, 97) for lo in (40, 47, 60)]
    out += [(f"WWWW inserted at {at}", seq[:at] + "WWWW" + seq[at:], 100.5, 104) for at in (30, 55)]
    out += [("three mutations", mut, 98.0, 104), ("mutations, deletion, ends removed", mut[5:50] + mut[57:-3], 78.0, 89)]
    return out


def test_alignment_equals_the_oracle_where_the_optimum_is_unique(seq):
    for name, other, score, n_pairs in cases(seq):
        best, n_ends, first, last = ao.local_align(seq, other)
        assert n_ends == 1 and first == last, f"{name}: the oracle finds this optimum ambiguous"
        assert best == score and len(first) == n_pairs, (name, best, len(first))
        got_score, blocks = sequence.local_alignment(seq, other)
        assert got_score == score, (name, got_score)
        assert ao.pairs_of_blocks(blocks) == first, name
        for (a0, a1), (b0, b1) in blocks:
            assert a1 - a0 == b1 - b0 > 0
        # gap-free blocks: consecutive blocks are separated by a gap on at least one side
        for (p, q), (r, s) in zip(blocks, blocks[1:]):
            assert (r[0] > p[1] or s[0] > q[1]) and r[0] >= p[1] and s[0] >= q[1]


def test_mismatches_stay_mapped(seq):
    _, blocks = sequence.local_alignment(seq, mutate(seq, (20, 21, 70)))
    assert blocks == [((0, 104), (0, 104))]


def test_random_sequences_score_like_the_oracle():
    rng = np.random.Generator(np.random.PCG64(7))
    for _ in range(300):
        a = "".join(rng.choice(list("ACDE"), size=int(rng.integers(1, 41))))
        b = "".join(rng.choice(list("ACDE"), size=int(rng.integers(1, 41))))
        got, blocks = sequence.local_alignment(a, b)
        want = ao.local_align(a, b)[0]
        assert got == want, (a, b, got, want)
        # the blocks are a valid alignment of that score
        score, prev = 0.0, None
        for (a0, a1), (b0, b1) in blocks:
            score += sum(1.0 if a[i] == b[j] else -1.0 for i, j in zip(range(a0, a1), range(b0, b1)))
            if prev is not None:
                for gap in (a0 - prev[0], b0 - prev[1]):
                    score -= (2.0 + 0.5 * (gap - 1)) if gap else 0.0
            prev = (a1, b1)
        assert score == got, (a, b, blocks)


def test_no_positive_score_and_empty_input():
    assert sequence.local_alignment("AAAA", "CCCC") == (0.0, [])
    assert sequence.local_alignment("", "ACD") == (0.0, [])


def test_documented_tie_rule_on_an_ambiguous_input():
    """Deleting AB out of ...ABAB... can be read as losing the first AB, the middle BA or the last AB: three co-optimal
    alignments.  The rule of sequence.py (smallest end cell; stop, then match before a gap in a before a gap in b while
    walking BACK) keeps the pairs next to the end of the alignment, so the gap lands as early as possible."""
    a, b = "CCCCCCABABDDDDDD", "CCCCCCABDDDDDD"
    best, n_ends, first, last = ao.local_align(a, b)
    assert best == 11.5 and first != last, "the oracle should find this input ambiguous"
    score, blocks = sequence.local_alignment(a, b)
    assert score == 11.5
    assert blocks == [((0, 6), (0, 6)), ((8, 16), (6, 14))]
    assert ao.pairs_of_blocks(blocks) == first
    # two end cells of equal score: the smallest (i, j) is taken
    best, n_ends, first, last = ao.local_align("ACDXXACD", "ACD")
    assert best == 3.0 and n_ends == 2
    assert sequence.local_alignment("ACDXXACD", "ACD") == (3.0, [((0, 3), (0, 3))])
    # a prefix that sums to zero is left out: the alignment starts where the rest of the score is 0
    assert sequence.local_alignment("AWCDE", "AYCDE") == (3.0, [((2, 5), (2, 5))])


def test_sequences_of_edited_topologies(top, seq):
    shifted = edited(top, np.arange(5, top.n_atoms), shift=500)
    letters, resids = sequence.residue_sequence(shifted)
    assert letters == seq[5:] and resids == list(range(1009, 1108))
    water = appended(top, "O", "HOH", "W", 900)
    letters, resids = sequence.residue_sequence(water)
    assert letters == seq + "X" and resids[-1] == 900
    # a residue ends where chain, resid or resname changes, and only there
    two = trajectory.Topology(["N", "CA", "N", "CA", "CA"], ["ALA", "ALA", "ALA", "ALA", "GLY"], ["A", "A", "B", "B", "B"], ["A"] * 5,
                              np.array([1, 1, 1, 1, 1]), np.zeros((5, 3), dtype=np.float32), None)
    assert sequence.residue_sequence(two) == ("AAG", [1, 1, 1])
    assert sequence.residue_sequence(edited(top))[0] == seq


def test_residue_map_and_common_resids(top, seq, fixture_files):
    shifted = edited(top, np.arange(5, top.n_atoms), shift=500)
    water = appended(top, "O", "HOH", "W", 900)
    m = sequence.ResidueMap(top, shifted)
    assert sorted(m.mapping) == list(range(509, 608))
    assert all(m.mapping[r] == (seq[r - 504], seq[r - 504], r + 500) for r in range(509, 608))
    assert m.map_residue(509) == 1009 and m.map_residue(504) is None and m.map_residue(1) is None
    assert sorted(sequence.ResidueMap(top, water).mapping) == list(range(504, 608))
    assert sequence.common_resids(top, [top, shifted, water]) == list(range(509, 608))
    assert sequence.common_resids(fixture_files[1], [fixture_files[1]]) == list(range(504, 608))   # paths are read
    assert sequence.common_resids(top, []) == []
    # against the oracle's pairs
    pairs = ao.local_align(seq, seq[5:])[2]
    assert [(504 + i, 1009 + j) for i, j in pairs] == [(r, m.mapping[r][2]) for r in sorted(m.mapping)]


def test_a_repeated_reference_resid_keeps_the_later_residue(top, seq):
    resids = top.resids.copy()
    resids[10] = resids[3]                      # residue 10 carries the number of residue 3
    ref = dataclasses.replace(top, resids=resids)
    m = sequence.ResidueMap(ref, top)
    assert len(m.mapping) == 103 and 514 not in m.mapping
    assert m.mapping[507] == (seq[10], seq[10], 514)


def all_atom(residues, drop_ca_of=()):
    names, resnames, resids = [], [], []
    for resid, resname in residues:
        atoms = ["CA"] if resname == "CA" else ["N", "H", "CA", "C", "O", "CB"]
        for a in atoms:
            if a == "CA" and resid in drop_ca_of:
                continue
            names.append(a); resnames.append(resname); resids.append(resid)
    n = len(names)
    return trajectory.Topology(names, resnames, ["A"] * n, ["A"] * n, np.asarray(resids, dtype=np.int64),
                               np.arange(3 * n, dtype=np.float32).reshape(n, 3), None)


def test_fit_atoms_are_protein_c_alphas_in_topology_order():
    residues = [(1, "ALA"), (2, "GLY"), (3, "HIE"), (4, "LYS"), (5, "CA")]   # the last is a calcium ion named CA
    t = all_atom(residues)
    ca = sequence.ca_atoms(t, [1, 2, 3, 4, 5])
    assert list(ca) == [2, 8, 14, 20]
    assert [t.names[i] for i in ca] == ["CA"] * 4 and "CA" not in {t.resnames[i] for i in ca}
    assert list(sequence.ca_atoms(t, [3, 1])) == [2, 14]            # topology order, whatever the order of the resids
    assert "HIE" in sequence.PROTEIN_RESNAMES and "HOH" not in sequence.PROTEIN_RESNAMES and "CA" not in sequence.PROTEIN_RESNAMES
    assert set(sequence.THREE_TO_ONE) <= sequence.PROTEIN_RESNAMES
    ref_fit, fit = sequence.fit_atoms(t, all_atom([(r + 10, n) for r, n in residues]), [1, 2, 4])
    assert list(ref_fit) == [2, 8, 20] and list(fit) == [2, 8, 20]
    with pytest.raises(ValueError, match=r"3 C-alpha atoms to fit in broken\.pdb and 4 in the reference"):
        sequence.fit_atoms(t, all_atom(residues, drop_ca_of=(2,)), [1, 2, 3, 4], what="broken.pdb")


def test_tool_refuses_without_a_device_and_its_own_input(fixture_files, tmp_path, monkeypatch, caplog):
    import os

    import torch

    from deep_cartograph_amd import tools

    dcd, pdb = fixture_files
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.DcvError, match="no CPU fallback"):
        tools.align_trajectories(dcd, pdb, output_folder=str(tmp_path / "out"))
    assert not os.path.exists(tmp_path / "out")
    with pytest.raises(ValueError, match="written over its input"):
        tools.align_trajectories(dcd, pdb, output_folder=os.path.dirname(dcd))
    with pytest.raises(ValueError, match="do not match"):
        tools.align_trajectories([dcd, dcd], [pdb, pdb, pdb], output_folder=str(tmp_path / "out"))
    with pytest.raises(FileNotFoundError):
        tools.align_trajectories(dcd, pdb, ref_topology=str(tmp_path / "missing.pdb"), output_folder=str(tmp_path / "out"))
    # no common residues: an error is logged and nothing is written, with or without a device
    other = str(tmp_path / "other.pdb")
    t = trajectory.read_topology(pdb)
    trajectory.write_topology(other, dataclasses.replace(t, resnames=["HOH"] * t.n_atoms))
    with caplog.at_level("ERROR"):
        assert tools.align_trajectories(dcd, pdb, ref_topology=other, output_folder=str(tmp_path / "out")) == ([], [])
    assert "No common residues" in caplog.text


def test_command_line_takes_the_reference_arguments(fixture_files, tmp_path, monkeypatch):
    from deep_cartograph_amd import align, tools

    seen = {}
    monkeypatch.setattr(tools, "align_trajectories", lambda *a, **k: seen.update(args=a, kwargs=k))
    dcd, pdb = fixture_files
    align.main(["-traj_data", dcd, dcd, "-top_data", pdb, "-ref_top", pdb, "-output", str(tmp_path), "-v"])
    assert seen["args"] == ([dcd, dcd], [pdb]) and seen["kwargs"] == {"ref_topology": pdb, "output_folder": str(tmp_path)}


def test_library_declares_the_entry_and_validates_on_the_host():
    """The refusals come before any launch, so they can be asked for without a device: the pointers are never followed."""
    assert "dcv_transform_frames" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dcv_transform_frames"][1]) == 13
    lib = _lib.load()
    assert lib.dcv_abi_version() == 5
    A, n = 10, 4
    x, t, o = 0x10000, 0x20000, 0x30000   # made-up addresses, far enough apart

    def call(xyz=x, n_frames=n, strides=(3 * A, 3, 1), n_atoms=A, rows=t, ldt=16, out=o, out_strides=(3 * A, 3, 1)):
        return lib.dcv_transform_frames(xyz, n_frames, *strides, n_atoms, rows, ldt, out, *out_strides, None)

    assert call(n_frames=0) == 0
    assert call(ldt=14) == -1 and b"ldt" in lib.dcv_last_error()
    assert call(ldt=15, n_frames=0) == 0
    assert call(xyz=None) == -1 and call(rows=None) == -1 and call(out=None) == -1
    assert call(n_atoms=0) == -1 and call(n_frames=-1) == -1
    assert call(strides=(-1, 3, 1)) == -1 and call(strides=(3 * A, 0, 1)) == -1 and call(strides=(3 * A, 3, -1)) == -1
    assert call(out_strides=(0, 3, 1)) == -1 and call(out_strides=(3 * A, 0, 1)) == -1 and call(out_strides=(3 * A, 3, 0)) == -1
    assert call(xyz=x + 2) == -1 and call(out=o + 1) == -1
    # element ranges from the strides: [x, x + 4 * 120) and the output's
    assert call(out=x) == -1 and b"overlap" in lib.dcv_last_error()
    assert call(out=x + 4 * (n * A * 3 - 1)) == -1
    assert call(out=x - 4 * (n * A * 3 - 1)) == -1
    assert call(xyz=x, out=x + 4, strides=(0, 1, 1), out_strides=(1, 1, 1), n_atoms=1) == -1   # 3 and 6 elements
    assert call(rows=o + 8 * 16) == -1 and b"transform rows" in lib.dcv_last_error()   # the rows inside the output
    assert call(rows=o - 8 * (3 * 16 + 15) + 8) == -1                                    # their last double on its first element
    assert call(n_frames=1 << 61) == -1
