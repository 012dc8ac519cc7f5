"""Matching sampled structures against reference structures on the device.

The reference's scripts/evaluate.py asks pymatgen on the host whether a sample reproduces the ground truth
(`test_structure_matching`: StructureMatcher().fit(ref_st, st), reported as match rate and RMSD). Here the final
state is matched where it already is (the kernel is csrc/match.hip; the definition is in include/chemeleon_hip.h
at chm_match_*):

    ref = Reference.from_atoms(test_structures)                       # held on the device, cell records once
    atoms = model.sample(text, 8, 512, noise="philox", match=Match(ref, ref_of=[0] * 512, require=True))
    model.last_match.match_rate, model.last_match.rms_mean            # over the whole batch
    atoms[0].info["match"]                                            # the structure's record as a dict

    report = match_states(natoms, a, x, lat, Match(ref), perm=True)   # device tensors -> numpy arrays

Per crystal: both cells are Niggli-reduced (chemeleon_amd.cell), the sample is scaled to the reference's volume,
every integer matrix with entries in {-1, 0, 1} and determinant +-1 that carries the one reduced cell onto the other
within `ltol` (relative lengths) and `angle_tol` (degrees) is a lattice mapping, and for each mapping every atom of
the rarest species is tried as the origin. A candidate survives when each reference atom's nearest sample atom of
its type lies within `stol` (a fraction of l = (V / n)^(1/3)) and no sample atom is taken twice; the survivor with
the smallest rms displacement (mean removed, in units of l) is the answer. The defaults are StructureMatcher's.

This is not a port of pymatgen, and how far the two agree (StructureMatcher.fit) has not been measured. Atom
counts must be equal: there is no reduction to a primitive cell, so a supercell does not match its primitive
reference (chemeleon_amd.primitive, primitive_states or sample(primitive=...), is the way round it: it runs first).
The pairing is the nearest-partner rule by default; Match(..., pairing="assignment") pairs the atoms of a candidate
whose nearest partners collide by the optimal assignment on the squared distances instead, as StructureMatcher does
("Matching a reference" and "Pairing by assignment"); at most 64 such candidates per crystal are
solved (flag many_assignments beyond that) and `n_assigned` says how many were.
"""

import threading
from typing import Optional, Sequence

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd import cell as _cell
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state, hip_device, int32_array

NO_REFERENCE, NO_LATTICE, SIZE, COMPOSITION, THIN, MANY_MAPPINGS = 1, 2, 4, 8, 16, 32
MANY_ASSIGNMENTS = 128
FLAG_NAMES = {NO_REFERENCE: "no_reference", NO_LATTICE: "no_lattice", SIZE: "size", COMPOSITION: "composition",
              THIN: "thin", MANY_MAPPINGS: "many_mappings", MANY_ASSIGNMENTS: "many_assignments"}
PAIRINGS = {"nearest": 0, "assignment": 1}  # CHM_MATCH_PAIRING_*
MAX_ASSIGN = 64
PAIR_FLAG_BITS = 0xffff    # a pair record's flags word: the CHM_MATCH_* bits ...
PAIR_ASSIGNED_SHIFT = 16   # ... and n_assigned above them (assignment pairing only)


def check_pairing(pairing) -> str:
    """`pairing` if it is "nearest" or "assignment"; ValueError otherwise."""
    if not isinstance(pairing, str) or pairing not in PAIRINGS:
        raise ValueError(f"pairing must be 'nearest' or 'assignment', got {pairing!r}")
    return pairing

RECORD_BYTES = 64
MAX_ATOMS = 256
MAX_MAPPINGS = 256
MAX_LTOL, MAX_STOL, MAX_ANGLE_TOL = 1.0, 1.0, 30.0
# the tolerances of the cell pass whose records the matcher reads (both lists, every caller)
MATCH_CELL_SYMPREC, MATCH_CELL_ANGLE_TOLERANCE = 0.1, 10.0


class Reference:
    """R reference structures packed like a state: natoms [R], atom_types int64 [NR], frac_coords float32 [NR,3],
    lattices float32 [R,3,3] (row vectors). They are copied to a device, and their cell records computed there,
    once per device, the first time a batch on that device is matched. Validated on the host (ValueError)."""

    def __init__(self, natoms, atom_types, frac_coords, lattices):
        try:
            nat = [int(n) for n in natoms]
        except (TypeError, ValueError):
            raise ValueError(f"natoms must be a list of atom counts, got {natoms!r}") from None
        if not nat or min(nat) < 1:
            raise ValueError("a Reference needs at least one structure of at least one atom")
        if max(nat) > MAX_ATOMS:
            raise ValueError(f"the matcher holds at most {MAX_ATOMS} atoms per structure, got {max(nat)}")
        types = np.ascontiguousarray(np.asarray(atom_types))
        if types.dtype.kind not in "iu":
            raise ValueError("atom_types must be integers")
        types = types.astype(np.int64)
        x = np.ascontiguousarray(np.asarray(frac_coords, dtype=np.float32))
        lat = np.ascontiguousarray(np.asarray(lattices, dtype=np.float32))
        N, R = sum(nat), len(nat)
        if types.shape != (N,) or x.shape != (N, 3) or lat.shape != (R, 3, 3):
            raise ValueError(f"reference shapes do not match natoms: atom_types {types.shape}, frac_coords {x.shape}, "
                             f"lattices {lat.shape} for {R} structures of {N} atoms")
        self.natoms, self.atom_types, self.frac_coords, self.lattices = tuple(nat), types, x, lat
        self._on = {}
        self._lock = threading.Lock()

    @classmethod
    def from_arrays(cls, natoms, atom_types, frac_coords, lattices) -> "Reference":
        return cls(natoms, atom_types, frac_coords, lattices)

    @classmethod
    def from_atoms(cls, atoms) -> "Reference":
        """From one ase.Atoms or a list of them (atomic numbers, scaled positions, cell)."""
        items = [atoms] if hasattr(atoms, "get_scaled_positions") else list(atoms)
        if not items:
            raise ValueError("a Reference needs at least one structure")
        return cls([len(a) for a in items], np.concatenate([np.asarray(a.numbers) for a in items]),
                   np.concatenate([np.asarray(a.get_scaled_positions(wrap=False)) for a in items]),
                   np.stack([np.asarray(a.cell) for a in items]))

    def __len__(self):
        return len(self.natoms)

    def on(self, device):
        """(atom_types, frac_coords, lattices, cell records) on `device`, made once per device."""
        dev = hip_device(device)
        with self._lock:
            held = self._on.get(dev.index)
            if held is None:
                with torch.cuda.device(dev):
                    a = torch.from_numpy(self.atom_types).to(dev)
                    x = torch.from_numpy(self.frac_coords).to(dev)
                    lat = torch.from_numpy(self.lattices).to(dev)
                    rec = torch.empty(len(self.natoms) * _cell.RECORD_BYTES, dtype=torch.uint8, device=dev)
                    _cell.cell_plan(self.natoms, dev).run(lat, None, MATCH_CELL_SYMPREC, MATCH_CELL_ANGLE_TOLERANCE, rec)
                    torch.cuda.current_stream(dev).synchronize()
                held = self._on[dev.index] = (a, x, lat, rec)
            return held


class Match:
    """How finished structures are matched: `reference` (a Reference), `ref_of` (one reference index per crystal,
    -1 for none; None = the one reference for every crystal, or crystal g against reference g when there are as
    many references as crystals), the tolerances `ltol` (relative length, at most 1), `stol` (fraction of
    (V / n)^(1/3), at most 1) and `angle_tol` (degrees, at most 30), and `require`: with True the crystals that do
    not match count as failed in sample() / finish_atoms; `pairing`: "nearest" (each reference atom takes its nearest
    sample atom, a candidate with a collision is given up) or "assignment" (a collided candidate is paired by the
    optimal assignment). Everything is validated here, on the host (ValueError)."""

    def __init__(self, reference: Reference, ref_of: Optional[Sequence[int]] = None, ltol: float = 0.2,
                 stol: float = 0.3, angle_tol: float = 5.0, require: bool = False, pairing: str = "nearest"):
        if not isinstance(reference, Reference):
            raise ValueError("reference must be a chemeleon_amd.Reference")
        self.pairing = check_pairing(pairing)
        for name, v, top in (("ltol", ltol, MAX_LTOL), ("stol", stol, MAX_STOL), ("angle_tol", angle_tol, MAX_ANGLE_TOL)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not 0 < float(np.float32(v)) <= top:
                raise ValueError(f"{name} must be in (0, {top:g}], got {v!r}")
        if not isinstance(require, (bool, np.bool_)):
            raise ValueError(f"require must be a bool, got {require!r}")
        self.reference = reference
        self.ltol, self.stol, self.angle_tol, self.require = float(ltol), float(stol), float(angle_tol), bool(require)
        if ref_of is None:
            self.ref_of = None
        else:
            try:
                of = [v for v in ref_of]
            except TypeError:
                raise ValueError(f"ref_of must be a list of reference indices, got {ref_of!r}") from None
            if not of:
                raise ValueError("ref_of: an empty list")
            for v in of:
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise ValueError(f"ref_of must hold integers, got {v!r}")
                if not -1 <= int(v) < len(reference):
                    raise ValueError(f"ref_of entry {int(v)} outside [-1, {len(reference)})")
            self.ref_of = tuple(int(v) for v in of)

    def ref_of_for(self, num_graphs: int) -> tuple:
        """The reference index of each crystal of a batch of num_graphs; ValueError if the list has another length
        or None cannot be resolved."""
        R = len(self.reference)
        if self.ref_of is None:
            if R == 1:
                return (0,) * num_graphs
            if R == num_graphs:
                return tuple(range(R))
            raise ValueError(f"ref_of=None needs one reference or one per crystal: {R} references, {num_graphs} crystals")
        if len(self.ref_of) != num_graphs:
            raise ValueError(f"ref_of lists {len(self.ref_of)} crystals, the batch has {num_graphs} crystals")
        return self.ref_of

    def __repr__(self):
        return (f"Match({len(self.reference)} references, ltol={self.ltol}, stol={self.stol}, angle_tol={self.angle_tol}, "
                f"require={self.require}" + (f", pairing={self.pairing!r})" if self.pairing != "nearest" else ")"))


class MatchReport:
    """The records of one batch as numpy arrays: matched [B] (bool), rms [B] (units of l), max_dist [B] (A), scale
    [B], l [B], mapping [B] (candidate index, -1), anchor [B] (-1), n_mappings, n_candidates, n_survivors [B],
    flags [B], ref [B], n_assigned [B] (candidates paired by assignment; 0 under "nearest"); n_matched, match_rate, rms_mean (over the matched crystals; nan if none), and mismatch [B]
    (= not matched). `perm` is None or, if asked for, int32 [N]: per crystal, at its node offset, the sample atom
    paired with each reference atom (-1 in a crystal that is not matched)."""

    def __init__(self, records: np.ndarray, perm: Optional[np.ndarray] = None):
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        f, i = rec.view(np.float32), rec.view(np.int32)
        self.records = rec
        self.rms, self.max_dist, self.scale, self.l = (f[:, k].copy() for k in range(4))
        self.mapping, self.anchor = i[:, 4].copy(), i[:, 5].copy()
        self.n_mappings, self.n_candidates, self.n_survivors = i[:, 6].copy(), i[:, 7].copy(), i[:, 8].copy()
        self.matched = i[:, 9] != 0
        self.flags, self.ref = i[:, 10].copy(), i[:, 11].copy()
        self.n_assigned = i[:, 12].copy()
        self.mismatch = ~self.matched
        self.n_matched = int(self.matched.sum())
        self.match_rate = self.n_matched / len(rec) if len(rec) else float("nan")
        self.rms_mean = float(self.rms[self.matched].astype(np.float64).mean()) if self.n_matched else float("nan")
        self.perm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)

    def __len__(self):
        return len(self.flags)

    def record(self, g: int) -> dict:
        """Crystal g's record as a dict of Python numbers (what sample() stores in atoms.info["match"])."""
        fl = int(self.flags[g])
        return {"matched": bool(self.matched[g]), "rms": float(self.rms[g]), "max_dist": float(self.max_dist[g]),
                "scale": float(self.scale[g]), "l": float(self.l[g]), "mapping": int(self.mapping[g]),
                "anchor": int(self.anchor[g]), "n_mappings": int(self.n_mappings[g]),
                "n_candidates": int(self.n_candidates[g]), "n_survivors": int(self.n_survivors[g]), "n_assigned": int(self.n_assigned[g]), "flags": fl,
                "failed": [name for bit, name in FLAG_NAMES.items() if fl & bit], "ref": int(self.ref[g])}


class MatchPlan(Plan):
    """Owns a chm_match: the node offsets of a crystal list and a reference list, and ref_of, on one device."""

    _create, _destroy = "chm_match_create", "chm_match_destroy"

    def __init__(self, natoms: Sequence[int], ref_natoms: Sequence[int], ref_of: Sequence[int], device):
        self.natoms, self.ref_natoms = tuple(int(n) for n in natoms), tuple(int(n) for n in ref_natoms)
        self.ref_of = tuple(int(r) for r in ref_of)
        self.device = torch.device(device)
        if len(self.ref_of) != len(self.natoms):
            raise ValueError(f"ref_of lists {len(self.ref_of)} crystals, natoms {len(self.natoms)}")
        self._make(int32_array(self.natoms), len(self.natoms), int32_array(self.ref_natoms), len(self.ref_natoms),
                   int32_array(self.ref_of))

    def run(self, cell_records, atom_types, frac_coords, lattices, ref_cell_records, ref_atom_types, ref_frac_coords,
            ref_lattices, ltol: float, stol: float, angle_tol: float, out, perm=None, pairing: str = "nearest"):
        """Enqueues the search on the current stream of the plan's device: the cell records are the outputs of
        CellPlan.run on the two lattice lists, `out` a uint8 device tensor of 64 bytes per crystal, `perm` None or
        an int32 device tensor [N]. No host wait."""
        _lib.check(_lib.load().chm_match_run_pairing(
            self.handle, _lib.ptr(cell_records), cell_records.numel(), _lib.ptr(atom_types), atom_types.numel(),
            _lib.ptr(frac_coords), frac_coords.numel(), _lib.ptr(lattices), lattices.numel(),
            _lib.ptr(ref_cell_records), ref_cell_records.numel(), _lib.ptr(ref_atom_types), ref_atom_types.numel(),
            _lib.ptr(ref_frac_coords), ref_frac_coords.numel(), _lib.ptr(ref_lattices), ref_lattices.numel(),
            float(ltol), float(stol), float(angle_tol), _lib.ptr(out), out.numel(), _lib.ptr(perm),
            0 if perm is None else perm.numel(), _lib.stream_handle(self.device), PAIRINGS[check_pairing(pairing)]),
            "chm_match_run_pairing")
        return out


_plans = PlanCache(MatchPlan)


def match_plan(natoms: Sequence[int], ref_natoms: Sequence[int], ref_of: Sequence[int], device) -> MatchPlan:
    """The plan of these lists on this device, cached per (natoms, ref_natoms, ref_of, device) (the last 8)."""
    return _plans.get(device, natoms, ref_natoms, ref_of)


def match_states(natoms: Sequence[int], atom_types, frac_coords, lattices, match: Match, perm: bool = False) -> MatchReport:
    """Matches a state that lives on the device (atom_types [N] int64, frac_coords [N,3] and lattices [B,3,3] fp32,
    in node order of `natoms`; at most 256 atoms per crystal) against match.reference and returns its MatchReport:
    the cell pass and the match pass are enqueued on one stream and only the 64-byte records (and the pairing, if
    asked for) cross to the host. CPU tensors are refused: there is no host path."""
    if not isinstance(match, Match):
        raise ValueError("match must be a chemeleon_amd.Match")
    nat = check_natoms(natoms, MAX_ATOMS, "the matcher")
    ref_of = match.ref_of_for(len(nat))
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices)
    ra, rx, rlat, rrec = match.reference.on(dev)
    cells, plan = _cell.cell_plan(nat, dev), match_plan(nat, match.reference.natoms, ref_of, dev)
    with torch.cuda.device(dev):
        cell_rec = torch.empty(B * _cell.RECORD_BYTES, dtype=torch.uint8, device=dev)
        out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
        pm = torch.empty(N, dtype=torch.int32, device=dev) if perm else None
        cells.run(lattices, None, MATCH_CELL_SYMPREC, MATCH_CELL_ANGLE_TOLERANCE, cell_rec)
        plan.run(cell_rec, atom_types, frac_coords, lattices, rrec, ra, rx, rlat, match.ltol, match.stol,
                 match.angle_tol, out, pm, match.pairing)
        host = out.cpu().numpy()  # (waits for the kernels; cell_rec and out stay alive until here)
        host_perm = pm.cpu().numpy() if perm else None
    return MatchReport(host, host_perm)
