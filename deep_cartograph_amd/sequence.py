"""Residue mapping between topologies on the host (align_trajectories): the one-letter sequence of a topology, a
local pairwise alignment of two sequences and the map from reference residue numbers to a target's.  NumPy only.

What the reference asks of Biopython (modules/bio/bio.py: PDBParser + seq1, PairwiseAligner in local mode with
match 1, mismatch -1, open_gap_score -2, extend_gap_score -0.5, ``alignment.aligned``), restated from the published
algorithm: Smith-Waterman with affine gaps in Gotoh's three-matrix form.

Unpinned choices (Biopython is not available to compare with), each fixed here and pinned by tests/test_align_cpu.py:

* **Co-optimal alignments.**  Biopython returns "the first" of its co-optimal alignments without documenting an
  order.  Here: the end cell is the one with the smallest (i, j), i first, among the cells of the best score; walking
  back, the alignment starts as soon as the remaining score is 0 (the shortest alignment), and otherwise a step is
  taken as a match / mismatch before a gap in ``a`` before a gap in ``b``.
* **Rare residue codes.**  Biopython's ``seq1`` also knows a few rarer three-letter codes (SEC -> U, PYL -> O, ASX ->
  B, GLX -> Z, XLE -> J); here everything outside the 20 standard names is ``X``, protonation variants such as HIE
  included, as in ``seq1``.
* **Protein residue names** of the C-alpha fit selection (`PROTEIN_RESNAMES`): the 20 standard names and their usual
  protonation / tautomer variants.  MDAnalysis's own list behind its ``backbone`` keyword is longer."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import trajectory

THREE_TO_ONE = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H", "ILE": "I",
                "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W", "TYR": "Y", "VAL": "V"}

# residues whose CA atom is a C-alpha: the standard names plus protonation states and tautomers of the common force fields
PROTEIN_RESNAMES = frozenset(THREE_TO_ONE) | frozenset({
    "HID", "HIE", "HIP", "HSD", "HSE", "HSP", "HIS1", "HIS2", "HISA", "HISB", "HISD", "HISE", "HISH",
    "ASH", "ASPH", "GLH", "GLUH", "LYN", "LYSH", "ARGN", "CYM", "CYX", "CYS1", "CYS2", "CYSH", "MSE"})

MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND = 1.0, -1.0, 2.0, 0.5   # a gap of length L costs GAP_OPEN + GAP_EXTEND (L - 1)

Blocks = List[Tuple[Tuple[int, int], Tuple[int, int]]]


def _as_topology(top) -> trajectory.Topology:
    return top if isinstance(top, trajectory.Topology) else trajectory.read_topology(top)


def residue_sequence(top) -> Tuple[str, List[int]]:
    """(one-letter sequence, residue numbers) of a topology (or a PDB path): the atoms are walked in file order and a
    new residue starts whenever (chain, resid, resname) changes.  The 20 standard residue names give their letter,
    anything else -- hetero residues, water and ions included, which stay in the sequence -- gives ``X``."""
    top = _as_topology(top)
    letters, resids = [], []
    last = None
    for chain, resid, resname in zip(top.chains, top.resids, top.resnames):
        key = (chain, int(resid), resname)
        if key != last:
            letters.append(THREE_TO_ONE.get(resname.upper(), "X"))
            resids.append(int(resid))
            last = key
    return "".join(letters), resids


def local_alignment(a: str, b: str) -> Tuple[float, Blocks]:
    """(score, blocks) of the best local alignment of ``a`` and ``b``: match +1, mismatch -1, a gap of length L costs
    2 + 0.5 (L - 1).  ``blocks`` are the gap-free aligned ranges ``((a_start, a_end), (b_start, b_end))``, ends
    exclusive, mismatched pairs included -- what Biopython's ``alignment.aligned`` holds.  No positive score: (0.0, []).
    The choice among co-optimal alignments is the module's rule (see above).  float64 matrices, O(len(a) len(b))."""
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return 0.0, []
    neg = -np.inf
    A = np.frombuffer(a.encode("utf-32-le"), dtype=np.uint32)
    B = np.frombuffer(b.encode("utf-32-le"), dtype=np.uint32)
    # M: ends in the pair (a[i-1], b[j-1]); Ga: ends in a gap in a (b[j-1] alone); Gb: ends in a gap in b (a[i-1] alone)
    M = np.full((n + 1, m + 1), neg)
    Ga = np.full((n + 1, m + 1), neg)
    Gb = np.full((n + 1, m + 1), neg)
    ramp = GAP_EXTEND * np.arange(m + 1, dtype=np.float64)   # multiples of 0.5: every sum below is exact
    for i in range(1, n + 1):
        s = np.where(B == A[i - 1], MATCH, MISMATCH)
        prev = np.maximum(np.maximum(M[i - 1, :-1], Ga[i - 1, :-1]), np.maximum(Gb[i - 1, :-1], 0.0))
        M[i, 1:] = s + prev
        Gb[i, 1:] = np.maximum(np.maximum(M[i - 1, 1:], Ga[i - 1, 1:]) - GAP_OPEN, Gb[i - 1, 1:] - GAP_EXTEND)
        # Ga[i, j] = max over k < j of (max(M, Gb)[i, k] - GAP_OPEN - GAP_EXTEND (j - k - 1)): a running maximum along the row
        opened = np.maximum(M[i, :-1], Gb[i, :-1]) - GAP_OPEN + ramp[:-1]
        Ga[i, 1:] = np.maximum.accumulate(opened) - ramp[:-1]
    score = float(M.max())
    if not score > 0.0:
        return 0.0, []
    i, j = (int(v) for v in np.argwhere(M == score)[0])   # row-major order: the smallest i, then the smallest j
    pairs = []
    state = "M"
    while True:
        if state == "M":
            pairs.append((i - 1, j - 1))
            rest = M[i, j] - (MATCH if a[i - 1] == b[j - 1] else MISMATCH)
            i, j = i - 1, j - 1
            if rest == 0.0:
                break
            state = "M" if rest == M[i, j] else ("Ga" if rest == Ga[i, j] else "Gb")
        elif state == "Ga":
            here = Ga[i, j]
            j -= 1
            state = "M" if here == M[i, j] - GAP_OPEN else ("Ga" if here == Ga[i, j] - GAP_EXTEND else "Gb")
        else:
            here = Gb[i, j]
            i -= 1
            state = "M" if here == M[i, j] - GAP_OPEN else ("Ga" if here == Ga[i, j] - GAP_OPEN else "Gb")
    pairs.reverse()
    blocks: Blocks = []
    for p, q in pairs:
        if blocks and blocks[-1][0][1] == p and blocks[-1][1][1] == q:
            blocks[-1] = ((blocks[-1][0][0], p + 1), (blocks[-1][1][0], q + 1))
        else:
            blocks.append(((p, p + 1), (q, q + 1)))
    return score, blocks


class ResidueMap:
    """The residues of ``top`` that the local alignment pairs with residues of ``ref_top`` (topologies or PDB paths).
    ``mapping``: {reference resid: (reference letter, letter, resid)}, filled block by block in alignment order; a
    reference resid that occurs twice keeps the later entry, as in the reference (bio.py:137-155)."""

    def __init__(self, ref_top, top):
        self.ref_sequence, self.ref_resids = residue_sequence(ref_top)
        self.sequence, self.resids = residue_sequence(top)
        self.score, self.blocks = local_alignment(self.ref_sequence, self.sequence)
        self.mapping: Dict[int, Tuple[str, str, int]] = {}
        for (r0, r1), (t0, t1) in self.blocks:
            for r, t in zip(range(r0, r1), range(t0, t1)):
                self.mapping[self.ref_resids[r]] = (self.ref_sequence[r], self.sequence[t], self.resids[t])

    def map_residue(self, ref_resid: int) -> Optional[int]:
        entry = self.mapping.get(int(ref_resid))
        return entry[2] if entry else None


def common_resids(ref_top, tops: Sequence) -> List[int]:
    """Sorted reference resids that the alignment maps into EVERY topology of ``tops`` (align_trajectories.py:17-49)."""
    if not tops:
        return []
    ref_top = _as_topology(ref_top)
    common = None
    for top in tops:
        mapped = set(ResidueMap(ref_top, top).mapping)
        common = mapped if common is None else common & mapped
    return sorted(common)


def ca_atoms(top, resids) -> np.ndarray:
    """Indices, in topology order, of the atoms named CA in a protein residue (`PROTEIN_RESNAMES`) whose resid is in
    ``resids``: the reference's ``backbone and name CA and resid ...`` built from the arrays (`select_atoms` refuses
    ``backbone``).  A calcium ion, also named CA, sits in a residue that is no protein residue and is left out."""
    top = _as_topology(top)
    wanted = {int(r) for r in resids}
    return np.asarray([i for i, (name, resname, resid) in enumerate(zip(top.names, top.resnames, top.resids))
                       if name == "CA" and resname.upper() in PROTEIN_RESNAMES and int(resid) in wanted], dtype=np.int64)


def fit_atoms(ref_top, top, common: Sequence[int], what: str = "the topology") -> Tuple[np.ndarray, np.ndarray]:
    """(reference atoms, target atoms) of the C-alpha fit: `ca_atoms` of the reference resids ``common`` in ``ref_top``
    and of the resids they map to in ``top``.  The two lists pair up in topology order (MDAnalysis with
    match_atoms=False), so they must be equally long: otherwise ValueError naming both counts and ``what``."""
    ref_top, top = _as_topology(ref_top), _as_topology(top)
    mapper = ResidueMap(ref_top, top)
    target = [r for r in (mapper.map_residue(r) for r in common) if r is not None]
    ref_fit, fit = ca_atoms(ref_top, common), ca_atoms(top, target)
    if len(fit) != len(ref_fit) or len(fit) == 0:
        raise ValueError(f"{len(fit)} C-alpha atoms to fit in {what} and {len(ref_fit)} in the reference topology: the fit atoms pair up "
                         "in topology order and must be equally many (and at least one)")
    return ref_fit, fit
