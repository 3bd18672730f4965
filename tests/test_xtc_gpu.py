"""The XTC decoder on the device: dcv_xtc_decode / hip.xtc_decode against the CPU oracle (tests/xtc_oracle.py) on the
reference's own files and on synthetic streams that reach every branch of the format, its guards on corrupt streams, its
host-side refusals, and the import step (tools.import_trajectories, compute_features on an ``.xtc``).

Bounds.  The decoded integers are exact and the two float32 multiplications of the conversion are the oracle's, so every
comparison is bit for bit (assert_array_equal)."""
import os

import numpy as np
import pytest
import torch

from deep_cartograph_amd import _lib
from tests import xtc_oracle as xo
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

NAN_BITS = np.uint32(0x7FC0BEEF)   # a NaN with a payload: no coordinate the kernel writes has these bits


@pytest.fixture(scope="module")
def golden():
    g = load_golden("xtc_golden.npz")
    return {"aladip": g["aladip_xtc"].tobytes(), "protein": g["protein_xtc"].tobytes(), "protein_pdb": str(g["protein_pdb"])}


@pytest.fixture(scope="module")
def decoded(golden):
    """The oracle's decode of both fixtures, computed once: {name: xyz [n, A, 3] float32, Angstrom}."""
    return {name: xo.decode(golden[name])[1] for name in ("aladip", "protein")}


def index_of(data: bytes, tmp_path, name="t.xtc"):
    from deep_cartograph_amd import trajectory as tr

    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return tr.index_xtc(path)


def upload(data: bytes, first=0, last=None) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8)[first:last].copy()).cuda()


def nan_buffer(words: int) -> torch.Tensor:
    return torch.from_numpy(np.full(words, NAN_BITS, dtype=np.uint32).view(np.float32)).cuda()


def bits(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------ the reference's own files
@pytest.mark.parametrize("name", ["aladip", "protein"])
def test_fixture_dense(name, golden, decoded, tmp_path):
    from deep_cartograph_amd import hip

    idx = index_of(golden[name], tmp_path)
    first, last, desc = idx.span(np.arange(idx.n_frames))
    got = hip.xtc_decode(upload(golden[name], first, last), desc, idx.n_atoms)
    assert got.shape == decoded[name].shape and got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy(), decoded[name])


@pytest.mark.parametrize("name", ["aladip", "protein"])
def test_fixture_into_dcd_records(name, golden, decoded, tmp_path):
    """Into the planes of DCD frame records inside a NaN-filled buffer: the record markers and everything around the image
    keep their bits."""
    from deep_cartograph_amd import hip, trajectory as tr

    idx = index_of(golden[name], tmp_path)
    n, A = idx.n_frames, idx.n_atoms
    writer = tr.write_dcd(str(tmp_path / "unused.dcd"), A)
    off, fs, as_, cs = writer.layout()
    writer.close()
    pad = 8
    out = nan_buffer(pad + n * fs + pad)
    first, last, desc = idx.span(np.arange(n))
    ret, status = hip.xtc_decode(upload(golden[name], first, last), desc, A, out=out, out_strides=(pad + off, fs, as_, cs), return_status=True)
    assert ret is out and not status.any()
    got = bits(out)
    slots = (pad + off + fs * np.arange(n)[:, None, None] + as_ * np.arange(A)[None, :, None] + cs * np.arange(3)[None, None, :])
    np.testing.assert_array_equal(got[slots].view(np.float32), decoded[name])
    rest = np.ones(got.size, dtype=bool)
    rest[slots.reshape(-1)] = False
    assert rest.sum() == 2 * pad + 6 * n and np.all(got[rest] == NAN_BITS)


@pytest.mark.parametrize("name", ["aladip", "protein"])
def test_fixture_every_third_frame(name, golden, decoded, tmp_path):
    from deep_cartograph_amd import hip

    idx = index_of(golden[name], tmp_path)
    keep = np.arange(1, idx.n_frames, 3)
    first, last, desc = idx.span(keep)
    assert first == idx.offset[1] and last - first < len(golden[name])
    got = hip.xtc_decode(upload(golden[name], first, last), desc, idx.n_atoms)
    np.testing.assert_array_equal(got.cpu().numpy(), decoded[name][keep])


def test_scale_is_the_second_multiplication(golden, tmp_path):
    from deep_cartograph_amd import hip

    idx = index_of(golden["protein"], tmp_path)
    first, last, desc = idx.span(np.arange(4))
    nm = hip.xtc_decode(upload(golden["protein"], first, last), desc, 457, scale=1.0).cpu().numpy()
    np.testing.assert_array_equal(nm, xo.decode(golden["protein"], scale=1.0)[1][:4])


# ------------------------------------------------------------------------------------------------ synthetic streams
@pytest.mark.parametrize("name", xo.CASES)
def test_synthetic_streams(name, tmp_path):
    """65 frames (two waves, one of them partial) of unequal byte length, nbytes no multiple of 4: the smallest compressed
    frame, the raw form, all eight run codes with the swap, a run that ends at the last atom, smallidx walked down to 9 and
    up to 72, flag = 0 behind a run, fields of up to 32 bits, a 72-bit unpack3, negative minint, precision 100."""
    from deep_cartograph_amd import hip

    data, ints, precision = xo.synthetic(name)
    _, want, status = xo.decode(data)
    assert not status.any()
    idx = index_of(data, tmp_path)
    assert idx.n_frames == 65
    first, last, desc = idx.span(np.arange(65))
    got = hip.xtc_decode(upload(data, first, last), desc, idx.n_atoms)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if ints is not None:
        np.testing.assert_array_equal(got.cpu().numpy(), xo.to_float(ints, precision))


# ------------------------------------------------------------------------------------------------ guards
def _corrupt_batch(golden):
    """(bytes, descriptors as the oracle takes them, halved frame, randomised frame): the protein fixture with frame 5's nbytes
    halved and frame 17's payload random.  The seed is the first whose random payload the CPU oracle marks."""
    frames = xo.frames(golden["protein"])
    frames[5] = dict(frames[5], nbytes=frames[5]["nbytes"] // 2)
    f = frames[17]
    for seed in range(16):
        buf = bytearray(golden["protein"])
        buf[f["offset"]:f["offset"] + f["nbytes"]] = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, f["nbytes"], dtype=np.uint8).tobytes()
        _, want, status = xo.decode(bytes(buf), descriptors=frames)
        if status[17] != 0:
            break
    else:
        raise AssertionError("no seed whose random payload is inconsistent")
    assert np.flatnonzero(status).tolist() == [5, 17] and status[5] == xo.SHORT
    return bytes(buf), frames, want


def test_guards_on_corrupt_streams(golden):
    """One frame with half its bytes and one with random bytes among 22 good ones.  The file bytes are followed, inside
    the same allocation, by a band of 0xFF bytes and the output by a NaN band: exactly the two frames are marked, every
    other frame is exact and both bands keep their bits."""
    from deep_cartograph_amd import hip

    data, frames, want = _corrupt_batch(golden)
    desc = np.zeros(24, dtype=_lib.XTC_FRAME_DTYPE)
    for i, f in enumerate(frames):
        desc[i] = (f["offset"], f["nbytes"], f["smallidx"], f["precision"], 0, f["minint"], f["maxint"])
    band = 4096
    whole = torch.from_numpy(np.concatenate([np.frombuffer(data, dtype=np.uint8), np.full(band, 0xFF, dtype=np.uint8)])).cuda()
    out = nan_buffer(24 * 457 * 3 + band)
    ret, status = hip.xtc_decode(whole[:len(data)], desc, 457, out=out, out_strides=(0, 3 * 457, 3, 1), return_status=True)
    status = status.cpu().numpy()
    assert np.flatnonzero(status).tolist() == [5, 17], status
    got = bits(out)
    xyz = got[:24 * 457 * 3].view(np.float32).reshape(24, 457, 3)
    good = np.setdiff1d(np.arange(24), [5, 17])
    np.testing.assert_array_equal(xyz[good], want[good])
    assert np.all(got[24 * 457 * 3:] == NAN_BITS)
    assert np.all(whole[len(data):].cpu().numpy() == 0xFF) and np.array_equal(whole[:len(data)].cpu().numpy(), np.frombuffer(data, dtype=np.uint8))
    for f in (5, 17):   # a marked frame: what it wrote before the inconsistency is what the oracle wrote, the rest is untouched
        written = ~np.isnan(want[f])
        np.testing.assert_array_equal(xyz[f][written], want[f][written])
        assert np.all(xyz[f].view(np.uint32)[~written] == NAN_BITS)
    with pytest.raises(_lib.DcvError, match=r"frame 5 of the 24 given did not decode: the stream needs bits behind its nbytes"):
        hip.xtc_decode(whole[:len(data)], desc, 457)


def test_header_guards_mark_the_frame(golden, tmp_path):
    """Descriptors no index would hand out: a smallidx outside [9, 72], maxint below minint, a precision of 0 and NaN."""
    from deep_cartograph_amd import hip

    idx = index_of(golden["protein"], tmp_path)
    first, last, desc = idx.span(np.arange(6))
    desc["smallidx"][1], desc["smallidx"][2] = 8, 73
    desc["maxint"][3, 1] = desc["minint"][3, 1] - 1
    desc["precision"][4], desc["precision"][5] = 0.0, np.nan
    out = nan_buffer(6 * 457 * 3)
    _, status = hip.xtc_decode(upload(golden["protein"], first, last), desc, 457, out=out, out_strides=(0, 3 * 457, 3, 1), return_status=True)
    assert status.cpu().numpy().tolist() == [0, 3, 3, 4, 4, 4]
    got = bits(out).reshape(6, -1)
    assert np.all(got[1:] == NAN_BITS)
    np.testing.assert_array_equal(got[0].view(np.float32).reshape(457, 3), xo.decode(golden["protein"])[1][0])


# ------------------------------------------------------------------------------------------------ host-side refusals
def _raw_call(data, desc, n_atoms, out, strides, status, ws, ws_bytes=None, n_bytes=None, n_frames=None):
    lib = _lib.load()
    return lib.dcv_xtc_decode(data.data_ptr(), data.numel() if n_bytes is None else n_bytes, desc.ctypes.data, len(desc) if n_frames is None else n_frames,
                              n_atoms, 10.0, out.data_ptr(), *strides, status.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                              torch.cuda.current_stream().cuda_stream)


def test_refusals_before_anything_is_launched(golden, tmp_path):
    idx = index_of(golden["protein"], tmp_path)
    first, last, desc = idx.span(np.arange(4))
    data = upload(golden["protein"], first, last)
    out = nan_buffer(4 * 457 * 3)
    status = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    need = lib.dcv_xtc_decode_workspace(4)
    assert need == 256 and lib.dcv_xtc_decode_workspace(6) == 512 and lib.dcv_xtc_decode_workspace(-1) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    dense = (3 * 457, 3, 1)

    def untouched():
        torch.cuda.synchronize()
        return np.all(bits(out) == NAN_BITS) and np.all(status.cpu().numpy() == -7)

    beyond = desc.copy()
    beyond["nbytes"][3] += 4                       # ends behind the uploaded bytes
    off_grid = desc.copy()
    off_grid["offset"][1] += 2
    negative = desc.copy()
    negative["offset"][0] = -4
    raw = desc.copy()
    raw["raw"][2] = 1                               # 457 atoms are not a raw frame
    for bad in (beyond, off_grid, negative, raw):
        assert _raw_call(data, bad, 457, out, dense, status, ws) == -1 and untouched()
    assert _raw_call(data, desc, 457, out, dense, status, ws, n_bytes=data.numel() - 4) == -1 and untouched()
    for strides in ((0, 3, 1), (3 * 457, 0, 1), (3 * 457, 3, 0), (3 * 457, 3, -1)):
        assert _raw_call(data, desc, 457, out, strides, status, ws) == -1 and untouched()
    assert _raw_call(data, desc, 0, out, dense, status, ws) == -1 and untouched()
    # an output that overlaps the input bytes: the same allocation, seen as float32
    both = torch.zeros(data.numel() + 4 * 4 * 457 * 3, dtype=torch.uint8, device="cuda")
    both[:data.numel()] = data
    inside = both[:data.numel()]
    overlapping = both[data.numel() - 16:].view(torch.float32)
    assert _raw_call(inside, desc, 457, overlapping, dense, status, ws) == -1
    assert b"overlap" in lib.dcv_last_error()
    assert _raw_call(data, desc, 457, out, dense, status, ws, ws_bytes=need - 1) == -3 and untouched()   # DCV_ENOMEM
    assert _raw_call(data, desc, 457, out, dense, status, ws, n_frames=0) == 0 and untouched()              # nothing to do
    assert _raw_call(data, desc, 457, out, dense, status, ws) == 0
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    np.testing.assert_array_equal(out.cpu().numpy().reshape(4, 457, 3), xo.decode(golden["protein"])[1][:4])


def test_wrapper_refusals(golden, tmp_path):
    from deep_cartograph_amd import hip

    idx = index_of(golden["protein"], tmp_path)
    first, last, desc = idx.span(np.arange(2))
    data = upload(golden["protein"], first, last)
    with pytest.raises(_lib.DcvError, match="XTC_FRAME_DTYPE"):
        hip.xtc_decode(data, np.zeros((2, 12), dtype=np.int32), 457)
    with pytest.raises(_lib.DcvError, match="uint8"):
        hip.xtc_decode(data.view(torch.int32), desc, 457)
    with pytest.raises(_lib.DcvError, match="reaches element"):
        hip.xtc_decode(data, desc, 457, out=nan_buffer(2 * 457 * 3 - 1), out_strides=(0, 3 * 457, 3, 1))
    with pytest.raises(_lib.DcvError, match="go together"):
        hip.xtc_decode(data, desc, 457, out=nan_buffer(2 * 457 * 3))
    empty, status = hip.xtc_decode(data, desc[:0], 457, return_status=True)
    assert tuple(empty.shape) == (0, 457, 3) and status.numel() == 0


# ------------------------------------------------------------------------------------------------ the import step
def _write_protein(golden, folder):
    os.makedirs(folder, exist_ok=True)
    xtc, pdb = os.path.join(folder, "protein.xtc"), os.path.join(folder, "protein.pdb")
    with open(xtc, "wb") as f:
        f.write(golden["protein"])
    with open(pdb, "w") as f:
        f.write(golden["protein_pdb"])
    return xtc, pdb


def test_import_trajectories(golden, decoded, tmp_path):
    from deep_cartograph_amd import tools, trajectory as tr

    xtc, _ = _write_protein(golden, str(tmp_path / "in"))
    paths = tools.import_trajectories([xtc, "other.dcd"], str(tmp_path / "whole"))
    assert paths == [str(tmp_path / "whole" / "protein.dcd"), "other.dcd"]
    traj = tr.open_trajectory(paths[0], 457)
    assert traj.n_frames == 24
    np.testing.assert_array_equal(traj.frames(), decoded["protein"])
    assert os.listdir(tmp_path / "whole") == ["protein.dcd"]   # the temporary name is gone
    one = tools.import_trajectories(xtc, str(tmp_path / "one_frame"), memory_budget=1)   # a budget of one frame a chunk
    assert open(one[0], "rb").read() == open(paths[0], "rb").read()
    rows = tools.import_trajectories([xtc], str(tmp_path / "rows"), traj_format="npy", traj_stride=5, memory_budget=40000)
    np.testing.assert_array_equal(np.load(rows[0]), decoded["protein"][::5])
    stamp = os.path.getmtime(paths[0])
    assert tools.import_trajectories([xtc], str(tmp_path / "whole")) == paths[:1] and os.path.getmtime(paths[0]) == stamp   # skipped


def test_import_reports_the_corrupt_frame(golden, tmp_path):
    from deep_cartograph_amd import tools

    data, frames, _ = _corrupt_batch(golden)   # frame 17's payload is random (frame 5's shorter nbytes is not in the file)
    path = str(tmp_path / "broken.xtc")
    with open(path, "wb") as f:
        f.write(data)
    with pytest.raises(_lib.DcvError, match=r"broken\.xtc: frames 0\.\.23 .*frame 17 of the 24 given did not decode"):
        tools.import_trajectories([path], str(tmp_path / "out"))
    assert os.listdir(tmp_path / "out") == []   # neither the trajectory nor its temporary file


def test_compute_features_from_xtc(golden, decoded, tmp_path):
    """Virtual dihedrals plus a distance group of the protein fixture: the ``.xtc`` gives, bit for bit, the matrix an
    ``.npy`` of the oracle's decode gives."""
    from deep_cartograph_amd import tools

    xtc, pdb = _write_protein(golden, str(tmp_path / "in"))
    npy = str(tmp_path / "in" / "decoded.npy")
    np.save(npy, decoded["protein"])
    features = {"dihedral_groups": {"tor": {"selection": "all", "periodic_encoding": True, "search_mode": "virtual"}},
                "distance_groups": {"dist": {"first_selection": "all", "second_selection": "all", "first_stride": 40, "second_stride": 50,
                                             "skip_neigh_residues": False, "skip_bonded_atoms": False}}}
    cfg = {"plumed_settings": {"traj_stride": 1, "features": features}}
    from_xtc = tools.compute_features(cfg, xtc, pdb, output_folder=str(tmp_path / "from_xtc"))
    from_npy = tools.compute_features(cfg, npy, pdb, output_folder=str(tmp_path / "from_npy"))
    assert from_xtc == [str(tmp_path / "from_xtc" / "protein" / "colvars.npy")]
    assert os.path.exists(tmp_path / "from_xtc" / "xtc_import" / "protein.dcd")
    a, b = np.load(from_xtc[0]), np.load(from_npy[0])
    assert a.shape == b.shape and a.shape[0] == 24 and a.shape[1] > 2 * 454
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
