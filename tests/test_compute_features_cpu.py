"""compute_features without a GPU: labels against PLUMED's own header lines, the heavy-atom / bond / neighbour rules on
tiny synthetic topologies, the selection parser, the DCD reader (the reference's file and files written here), the
schema, and the float64 oracle (tests/features_oracle.py) against both PLUMED-produced matrices."""
import json
import os
import struct

import numpy as np
import pytest

from tests import features_oracle as fo
from tests.conftest import load_golden

VIRTUAL_DIHEDRALS = {"dihedral_groups": {"tor": {"selection": "all", "periodic_encoding": True, "search_mode": "virtual"}}}
DISTANCES = {"distance_groups": {"dist": {"first_selection": "all", "second_selection": "all", "first_stride": 1, "second_stride": 10,
                                          "skip_neigh_residues": False, "skip_bonded_atoms": True}}}


@pytest.fixture(scope="module")
def golden():
    g, f = load_golden("compute_features_golden.npz"), load_golden("filter_golden.npz")
    return {"dcd": g["dcd"].tobytes(), "pdb": str(g["pdb"]), "distances": np.ascontiguousarray(g["distances"]),
            "distance_names": [str(s) for s in g["distance_names"]], "schema_defaults": json.loads(str(g["schema_defaults"])),
            "dihedrals": np.ascontiguousarray(f["X"]), "dihedral_names": [str(s) for s in f["names"]]}


@pytest.fixture(scope="module")
def fixture_files(golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("ca_example")
    dcd, pdb = str(d / "CA_example.dcd"), str(d / "CA_example.pdb")
    with open(dcd, "wb") as f:
        f.write(golden["dcd"])
    with open(pdb, "w") as f:
        f.write(golden["pdb"])
    return dcd, pdb


def pdb_line(serial, name, resname, chain, resid, x, y, z, record="ATOM"):
    return "%-6s%5d %-4s %-3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00\n" % (record, serial, name.ljust(3).rjust(4) if len(name) < 4 else name,
                                                                        resname, chain, resid, x, y, z)


def write_pdb(path, atoms, conect=()):
    with open(path, "w") as f:
        for i, a in enumerate(atoms):
            f.write(pdb_line(i + 1, *a))
        for rec in conect:
            f.write("CONECT" + "".join("%5d" % s for s in rec) + "\n")
        f.write("END\n")
    return str(path)


# ------------------------------------------------------------------------------------------------ labels
def test_labels_equal_plumed_headers(golden, fixture_files):
    from deep_cartograph_amd import trajectory as tr

    top = tr.read_topology(fixture_files[1])
    assert top.n_atoms == 104 and top.bonds is None
    names, defs = tr.feature_definitions(VIRTUAL_DIHEDRALS, top)
    assert names == golden["dihedral_names"] and len(names) == 202
    assert defs.shape == (101, 6) and defs.dtype == np.int32
    assert (defs[:, 0] == 1).all() and np.array_equal(defs[:, 5], 2 * np.arange(101))
    assert np.array_equal(defs[:, 1:5], np.arange(101)[:, None] + np.arange(4)[None, :])
    names, defs = tr.feature_definitions(DISTANCES, top)
    assert names == golden["distance_names"] and len(names) == 1078
    assert (defs[:, 0] == 0).all() and np.array_equal(defs[:, 5], np.arange(1078))
    # both kinds in one configuration: distance groups first, then dihedral groups
    names, defs = tr.feature_definitions({**VIRTUAL_DIHEDRALS, **DISTANCES}, top)
    assert names == golden["distance_names"] + golden["dihedral_names"]
    assert defs[1078, 5] == 1078 and defs[-1, 5] == 1078 + 200


def test_plain_angle_labels(fixture_files):
    from deep_cartograph_amd import trajectory as tr

    top = tr.read_topology(fixture_files[1])
    names, defs = tr.feature_definitions({"dihedral_groups": {"t": {"selection": "resid 504:508", "periodic_encoding": False,
                                                                     "search_mode": "virtual"}}}, top)
    assert names == ["tor-@CA_504-@CA_505-@CA_506-@CA_507", "tor-@CA_505-@CA_506-@CA_507-@CA_508"]
    assert defs.tolist() == [[2, 0, 1, 2, 3, 0], [2, 1, 2, 3, 4, 1]]


def test_heavy_atom_rules_and_the_virtual_dihedral_quirk(tmp_path):
    """Distances use heavy atoms only.  Virtual dihedrals COUNT the heavy atoms but index the selection before the
    hydrogens were removed (reference md.py:265-268): with N, H, CA, HA, C, O (4 heavy of 6) the single dihedral is
    N-H-CA-HA, not N-CA-C-O."""
    from deep_cartograph_amd import trajectory as tr

    atoms = [("N", "ALA", "A", 1, 0, 0, 0), ("H", "ALA", "A", 1, 1, 0, 0), ("CA", "ALA", "A", 1, 4, 0, 0),
             ("HA", "ALA", "A", 1, 4, 1, 0), ("C", "ALA", "A", 1, 8, 0, 0), ("O", "ALA", "A", 1, 12, 0, 0)]
    top = tr.read_topology(write_pdb(tmp_path / "h.pdb", atoms))
    assert top.names == ["N", "H", "CA", "HA", "C", "O"]
    names, defs = tr.feature_definitions({"distance_groups": {"d": {"first_selection": "all", "second_selection": "all", "first_stride": 1,
                                                                    "second_stride": 1, "skip_bonded_atoms": False}}}, top)
    assert names == ["dist-@N_1-@CA_1", "dist-@N_1-@C_1", "dist-@N_1-@O_1", "dist-@CA_1-@C_1", "dist-@CA_1-@O_1", "dist-@C_1-@O_1"]
    assert defs[:, 1:3].tolist() == [[0, 2], [0, 4], [0, 5], [2, 4], [2, 5], [4, 5]]
    # strides apply after the hydrogens are dropped: heavy atoms [N, CA, C, O][::2] = [N, C]
    names, _ = tr.feature_definitions({"distance_groups": {"d": {"first_selection": "all", "second_selection": "all", "first_stride": 2,
                                                                 "second_stride": 1, "skip_bonded_atoms": False}}}, top)
    assert names == ["dist-@N_1-@CA_1", "dist-@N_1-@C_1", "dist-@N_1-@O_1", "dist-@C_1-@CA_1", "dist-@C_1-@O_1"]
    names, defs = tr.feature_definitions({"dihedral_groups": {"t": {"selection": "all", "search_mode": "virtual"}}}, top)
    assert names == ["sin-@N_1-@H_1-@CA_1-@HA_1", "cos-@N_1-@H_1-@CA_1-@HA_1"]
    assert defs.tolist() == [[1, 0, 1, 2, 3, 0]]


def test_conect_bonds_against_the_distance_rule(tmp_path):
    """With CONECT records only those pairs are bonded; without them a pair closer than 2.0 A is."""
    from deep_cartograph_amd import trajectory as tr

    atoms = [("CA", "GLY", "A", 1, 0, 0, 0), ("CB", "GLY", "A", 2, 1.5, 0, 0), ("CG", "GLY", "A", 3, 3.0, 0, 0), ("CD", "GLY", "A", 4, 6.0, 0, 0)]
    group = {"first_selection": "all", "second_selection": "all", "first_stride": 1, "second_stride": 1, "skip_bonded_atoms": True}
    top = tr.read_topology(write_pdb(tmp_path / "nobonds.pdb", atoms))
    assert top.bonds is None
    names, _ = tr.feature_definitions({"distance_groups": {"d": group}}, top)
    # 0-1 and 1-2 are 1.5 A apart: guessed bonded
    assert names == ["dist-@CA_1-@CG_3", "dist-@CA_1-@CD_4", "dist-@CB_2-@CD_4", "dist-@CG_3-@CD_4"]
    top = tr.read_topology(write_pdb(tmp_path / "bonds.pdb", atoms, conect=[(1, 2), (2, 1), (3, 4), (4, 3)]))
    assert top.bonds == {(0, 1), (2, 3)}
    names, _ = tr.feature_definitions({"distance_groups": {"d": group}}, top)
    # 1-2 is close but not in CONECT: kept; 2-3 is 3.0 A apart but in CONECT: skipped
    assert names == ["dist-@CA_1-@CG_3", "dist-@CA_1-@CD_4", "dist-@CB_2-@CG_3", "dist-@CB_2-@CD_4"]
    names, _ = tr.feature_definitions({"distance_groups": {"d": {**group, "skip_bonded_atoms": False}}}, top)
    assert len(names) == 6
    # CONECT records without partners, or without any field, name no bond
    top = tr.read_topology(write_pdb(tmp_path / "lonely.pdb", atoms, conect=[(1,), (), (3, 4)]))
    assert top.bonds == {(2, 3)}


def test_skip_neighbouring_residues(tmp_path):
    from deep_cartograph_amd import trajectory as tr

    atoms = [("CA", "GLY", "A", r, 10.0 * r, 0, 0) for r in (1, 2, 3, 5)] + [("CB", "GLY", "A", 5, 55.0, 0, 0)]
    top = tr.read_topology(write_pdb(tmp_path / "n.pdb", atoms))
    group = {"first_selection": "all", "second_selection": "all", "first_stride": 1, "second_stride": 1, "skip_bonded_atoms": False,
             "skip_neigh_residues": True}
    names, _ = tr.feature_definitions({"distance_groups": {"d": group}}, top)
    assert names == ["dist-@CA_1-@CA_3", "dist-@CA_1-@CA_5", "dist-@CA_1-@CB_5", "dist-@CA_2-@CA_5", "dist-@CA_2-@CB_5",
                     "dist-@CA_3-@CA_5", "dist-@CA_3-@CB_5"]


def test_topology_stops_at_first_model_and_reads_hetatm(tmp_path):
    from deep_cartograph_amd import trajectory as tr

    path = tmp_path / "m.pdb"
    with open(path, "w") as f:
        f.write("MODEL        1\n" + pdb_line(1, "CA", "ALA", "A", 7, 1, 2, 3) + pdb_line(2, "ZN", "ZN", "B", 8, 4, 5, 6, record="HETATM"))
        f.write("ENDMDL\nMODEL        2\n" + pdb_line(1, "CA", "ALA", "A", 7, 9, 9, 9) + "ENDMDL\n")
    top = tr.read_topology(str(path))
    assert top.n_atoms == 2 and top.names == ["CA", "ZN"] and top.resnames == ["ALA", "ZN"] and top.chains == ["A", "B"]
    assert top.resids.tolist() == [7, 8] and np.array_equal(top.positions, np.array([[1, 2, 3], [4, 5, 6]], dtype=np.float32))


# ------------------------------------------------------------------------------------------------ selections
@pytest.fixture(scope="module")
def small_top(tmp_path_factory):
    from deep_cartograph_amd import trajectory as tr

    atoms = [("N", "ALA", "A", 1, 0, 0, 0), ("H", "ALA", "A", 1, 0, 0, 0), ("CA", "ALA", "A", 1, 0, 0, 0), ("CB", "ALA", "A", 1, 0, 0, 0),
             ("N", "GLY", "A", 2, 0, 0, 0), ("CA", "GLY", "A", 2, 0, 0, 0), ("HA2", "GLY", "A", 2, 0, 0, 0),
             ("N", "LYS", "B", 3, 0, 0, 0), ("CA", "LYS", "B", 3, 0, 0, 0), ("CA", "LEU", "B", 10, 0, 0, 0)]
    return tr.read_topology(write_pdb(tmp_path_factory.mktemp("sel") / "s.pdb", atoms))


@pytest.mark.parametrize("selection,expected", [
    ("all", list(range(10))),
    ("name CA", [2, 5, 8, 9]),
    ("name CA CB", [2, 3, 5, 8, 9]),
    ("name C*", [2, 3, 5, 8, 9]),
    ("not name H*", [0, 2, 3, 4, 5, 7, 8, 9]),
    ("resname GLY LYS", [4, 5, 6, 7, 8]),
    ("resname L*", [7, 8, 9]),
    ("segid B", [7, 8, 9]),
    ("chainID A and name N", [0, 4]),
    ("resid 2", [4, 5, 6]),
    ("resid 1 3", [0, 1, 2, 3, 7, 8]),
    ("resid 2:3", [4, 5, 6, 7, 8]),
    ("resid 2-10 and name CA", [5, 8, 9]),
    ("name CA or name N and resid 1", [0, 2, 5, 8, 9]),           # and binds tighter than or
    ("(name CA or name N) and resid 1", [0, 2]),
    ("not (name CA or name N)", [1, 3, 6]),
    ("not name CA and not name N", [1, 3, 6]),
    ("name CA and not (resid 1:2 or chainID B)", []),
])
def test_selection_forms(small_top, selection, expected):
    from deep_cartograph_amd import trajectory as tr

    assert tr.select_atoms(small_top, selection).tolist() == expected


@pytest.mark.parametrize("selection,token", [("protein", "protein"), ("name CA and backbone", "backbone"), ("around 5 name CA", "around"),
                                             ("name C?", "C?"), ("resid 1 to 5", "to"), ("index 0:3", "index"), ("name *A", "*A")])
def test_unsupported_selection_names_the_token(small_top, selection, token):
    from deep_cartograph_amd import trajectory as tr

    with pytest.raises(ValueError, match=r"'%s'" % token.replace("?", r"\?").replace("*", r"\*")):
        tr.select_atoms(small_top, selection)


# ------------------------------------------------------------------------------------------------ DCD reader
def write_dcd(path, xyz, cell=False, endian="<", fixed=0, four_d=0, nset=None, truncate=0, charmm=24):
    """A CHARMM-format DCD written field by field; xyz is (n, A, 3) float32."""
    n, A = xyz.shape[:2]
    icntrl = [0] * 20
    icntrl[0] = n if nset is None else nset
    icntrl[1], icntrl[2], icntrl[8], icntrl[10], icntrl[11], icntrl[19] = 1, 1, fixed, int(cell), four_d, charmm
    e = endian
    blob = struct.pack(e + "i4s20ii", 84, b"CORD", *icntrl, 84)
    title = b"written by the test".ljust(80)
    blob += struct.pack(e + "ii80si", 84, 1, title, 84)
    blob += struct.pack(e + "iii", 4, A, 4)
    for f in range(n):
        if cell:
            blob += struct.pack(e + "i6di", 48, 50.0, 0.0, 50.0, 0.0, 0.0, 50.0, 48)
        for c in range(3):
            blob += struct.pack(e + "i", 4 * A) + xyz[f, :, c].astype(e + "f4").tobytes() + struct.pack(e + "i", 4 * A)
    with open(path, "wb") as fh:
        fh.write(blob[:len(blob) - truncate])
    return str(path)


def test_dcd_reader_on_the_reference_file(fixture_files):
    from deep_cartograph_amd import trajectory as tr

    t = tr.open_trajectory(fixture_files[0], 104)
    assert (t.n_frames, t.n_atoms) == (164, 104)
    assert (t.atom_stride, t.comp_stride) == (1, 106)
    xyz = t.frames()
    assert xyz.shape == (164, 104, 3) and xyz.dtype == np.float32 and np.isfinite(xyz).all()
    # consecutive CA atoms stay a virtual bond apart in every frame: the planes were addressed as planes
    d = np.linalg.norm(np.diff(xyz.astype(np.float64), axis=1), axis=2)
    assert 3.0 < d.min() and d.max() < 4.6
    n, off, fs, as_, cs = t.layout(2, None, 3)
    assert n == 54 and fs == 3 * t.frame_stride and off == t.offset + 2 * t.frame_stride
    assert np.array_equal(t.frames(2, None, 3), xyz[2::3])
    span, lay = t.span(5, 12, 2)
    assert lay[0] == 4 and span[lay[1]] == xyz[5, 0, 0] and span[lay[1] + 3 * lay[2] + 103 * lay[3] + 2 * lay[4]] == xyz[11, 103, 2]
    assert span.size == lay[1] + 3 * lay[2] + 103 + 2 * 106 + 1
    with pytest.raises(ValueError, match="104 atoms in the trajectory, 103 in the topology"):
        tr.open_trajectory(fixture_files[0], 103)


@pytest.mark.parametrize("cell", [False, True])
@pytest.mark.parametrize("A", [4, 7])
def test_dcd_reader_on_written_files(tmp_path, cell, A):
    from deep_cartograph_amd import trajectory as tr

    rng = np.random.Generator(np.random.PCG64(A + cell))
    xyz = rng.standard_normal((5, A, 3)).astype(np.float32) * 10
    t = tr.open_trajectory(write_dcd(tmp_path / "w.dcd", xyz, cell=cell), A)
    assert (t.n_frames, t.n_atoms, t.comp_stride) == (5, A, A + 2)
    assert t.frame_stride == 3 * (A + 2) + (14 if cell else 0)
    assert np.array_equal(t.frames(), xyz)


def test_dcd_reader_refusals(tmp_path):
    from deep_cartograph_amd import trajectory as tr

    xyz = np.arange(3 * 4 * 3, dtype=np.float32).reshape(3, 4, 3)
    with pytest.raises(ValueError, match="truncated"):
        tr.open_trajectory(write_dcd(tmp_path / "t.dcd", xyz, truncate=20))
    with pytest.raises(ValueError, match="do not match the header's 5 frames"):
        tr.open_trajectory(write_dcd(tmp_path / "n.dcd", xyz, nset=5))
    with pytest.raises(ValueError, match="big-endian"):
        tr.open_trajectory(write_dcd(tmp_path / "b.dcd", xyz, endian=">"))
    with pytest.raises(ValueError, match="fixed atoms"):
        tr.open_trajectory(write_dcd(tmp_path / "f.dcd", xyz, fixed=2))
    with pytest.raises(ValueError, match="4th-dimension"):
        tr.open_trajectory(write_dcd(tmp_path / "d.dcd", xyz, four_d=1))
    with open(tmp_path / "x.dcd", "wb") as f:
        f.write(b"\0" * 200)
    with pytest.raises(ValueError, match="not a DCD"):
        tr.open_trajectory(str(tmp_path / "x.dcd"))
    with pytest.raises(ValueError, match="XTC"):
        tr.open_trajectory(str(tmp_path / "a.xtc"))


def test_npy_trajectory(tmp_path):
    from deep_cartograph_amd import trajectory as tr

    xyz = np.arange(6 * 5 * 3, dtype=np.float32).reshape(6, 5, 3)
    np.save(tmp_path / "a.npy", xyz)
    t = tr.open_trajectory(str(tmp_path / "a.npy"), 5)
    assert (t.n_frames, t.n_atoms, t.offset, t.frame_stride, t.atom_stride, t.comp_stride) == (6, 5, 0, 15, 3, 1)
    assert np.array_equal(t.frames(1, 6, 2), xyz[1:6:2])
    np.save(tmp_path / "b.npy", xyz.astype(np.float64))
    with pytest.raises(ValueError, match="float32"):
        tr.open_trajectory(str(tmp_path / "b.npy"))
    with pytest.raises(ValueError, match="5 atoms in the trajectory, 4 in the topology"):
        tr.open_trajectory(str(tmp_path / "a.npy"), 4)


# ------------------------------------------------------------------------------------------------ schema, scope, tool
def test_schema_defaults(golden):
    from deep_cartograph_amd.schemas import ComputeFeaturesSchema, DihedralGroup, DistanceGroup

    dump = ComputeFeaturesSchema().model_dump()
    assert dump.pop("colvars_format") == "npy"   # this project's one extension of the reference's schema
    assert json.loads(json.dumps(dump)) == golden["schema_defaults"]
    assert DistanceGroup().model_dump() == {"first_selection": "not name H*", "second_selection": "not name H*", "first_stride": 1,
                                            "second_stride": 5, "skip_neigh_residues": False, "skip_bonded_atoms": True}
    assert DihedralGroup().model_dump() == {"selection": "not name H*", "periodic_encoding": True, "search_mode": "real"}
    cfg = ComputeFeaturesSchema(plumed_settings={"timeout": 5, "features": VIRTUAL_DIHEDRALS}, plumed_environment={"bin_path": "/x/plumed"}).model_dump()
    assert cfg["plumed_settings"]["features"]["dihedral_groups"]["tor"]["search_mode"] == "virtual"


@pytest.mark.parametrize("features,word", [
    ({"coordinate_groups": {"c": {"selection": "all"}}}, "coordinate_groups"),
    ({"distance_to_center_groups": {"c": {"selection": "all", "center_selection": "all"}}}, "distance_to_center_groups"),
    ({"dihedral_groups": {"t": {"selection": "all", "search_mode": "real"}}}, "search_mode 'real'"),
    ({"dihedral_groups": {"t": {"selection": "all", "search_mode": "protein_backbone"}}}, "search_mode 'protein_backbone'"),
    ({"dihedral_groups": {"t": {"selection": "all"}}}, "search_mode 'real'"),     # the schema's default
    ({}, "No features found"),
])
def test_unsupported_feature_groups_raise(fixture_files, features, word):
    from deep_cartograph_amd import trajectory as tr

    with pytest.raises(ValueError, match=word):
        tr.feature_definitions(features, tr.read_topology(fixture_files[1]))


def test_tool_raises_without_a_gpu(fixture_files, tmp_path, monkeypatch):
    import torch

    from deep_cartograph_amd import tools
    from deep_cartograph_amd._lib import DcvError

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(DcvError, match="no CPU fallback"):
        tools.compute_features({"plumed_settings": {"features": VIRTUAL_DIHEDRALS}}, [fixture_files[0]], [fixture_files[1]],
                               output_folder=str(tmp_path / "cf"))
    assert not os.path.exists(tmp_path / "cf" / "CA_example" / "colvars.npy")


def test_cli_requires_colvars_or_trajectories(capsys):
    from deep_cartograph_amd import deep_carto

    with pytest.raises(SystemExit):
        deep_carto.main(["-conf", "none.yml"])
    assert "one of -colvars or -traj is required" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        deep_carto.main(["-conf", "none.yml", "-traj", "a.dcd"])
    assert "-traj needs -top" in capsys.readouterr().err


def test_colvars_and_trajectories_together_are_refused(tmp_path):
    from deep_cartograph_amd import deep_carto

    with pytest.raises(ValueError, match="either colvars_paths or trajectory_data"):
        deep_carto.deep_cartograph({}, ["a.npy"], trajectory_data=["a.dcd"], topology_data=["a.pdb"], output_folder=str(tmp_path / "o"))


# ------------------------------------------------------------------------------------------------ the oracle vs PLUMED
def test_oracle_reproduces_plumed_within_its_print_rounding(golden, fixture_files):
    """PLUMED printed both matrices with %.4f, so the printed value is within 5e-5 of what PLUMED computed; the float64
    oracle must be within 5e-5 of every printed value.  The goldens hold those decimals as float32 (at most 2.4e-7 away);
    rounding back to 4 decimals recovers the printed value exactly.  Measured: 4.99998e-5 (dihedrals), 4.99995e-5
    (distances)."""
    from deep_cartograph_amd import trajectory as tr

    top = tr.read_topology(fixture_files[1])
    xyz = tr.open_trajectory(fixture_files[0], top.n_atoms).frames()
    for features, printed in ((VIRTUAL_DIHEDRALS, golden["dihedrals"]), (DISTANCES, golden["distances"])):
        _, defs = tr.feature_definitions(features, top)
        got = fo.featurize(xyz, defs)
        printed = np.round(printed.astype(np.float64), 4)
        assert got.shape == printed.shape
        err = np.abs(got - printed).max()
        print("oracle vs PLUMED: max error %.6e over %d entries" % (err, got.size))
        assert err <= 5e-5 + 1e-12   # 1e-12: the printed decimals are not exact in binary


def test_oracle_conventions():
    xyz = np.zeros((1, 8, 3), dtype=np.float32)
    xyz[0, :4] = [[1, 0, 0], [0, 0, 0], [0, 0, 1], [0, 1, 1]]             # a +90 degree torsion in PLUMED's convention
    xyz[0, 4:] = [[0, 0, 0], [1, 1, 1], [2, 2, 2], [5, 5, 5]]             # collinear
    out = fo.featurize(xyz, [[1, 0, 1, 2, 3, 0], [2, 0, 1, 2, 3, 2], [1, 4, 5, 6, 7, 3], [2, 4, 5, 6, 7, 5], [0, 4, 7, 0, 0, 6], [0, 5, 5, 0, 0, 7],
                             [1, 4, 5, 5, 6, 8]], unit=1.0)
    assert out[0, 0] == 1.0 and out[0, 1] == 0.0 and out[0, 2] == np.pi / 2
    assert out[0, 3:6].tolist() == [0.0, 1.0, 0.0]
    assert out[0, 6] == np.sqrt(75.0) and out[0, 7] == 0.0
    assert out[0, 8:10].tolist() == [0.0, 1.0]                             # coincident middle atoms
    assert fo.ulp_distance_f32(np.float32([1.0, -1.0, 0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -1.0, -0.0])).tolist() == [1, 0, 0]
