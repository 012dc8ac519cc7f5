"""Grouping of duplicate samples on the device by pairwise structure matching and the leader rule.

The reference's workflows end with a uniqueness step (`test_unique` of scripts/evaluate.py and the grouping of
scripts/navigate_chemical_system.py, both pymatgen's `StructureMatcher().group_structures` on the host).
chemeleon_amd.dedup answers it with radial fingerprints; here two crystals of a batch are duplicates when they
match under the definition of chemeleon_amd.match (include/chemeleon_hip.h at chm_match_* and chm_match_group_*;
the kernels are csrc/match.hip), with its tolerances ltol / stol / angle_tol:

    atoms = model.sample("TiO2", 12, 512, noise="philox", dedup=MatchDedup())
    model.last_dedup.n_groups        # how many different crystals; `atoms` holds one representative of each
    atoms[0].info["dedup"]           # {"index", "group", "multiplicity", "rms"}

    report = match_group_states(natoms, a, x, lat, MatchDedup(stol=0.2))   # device tensors -> numpy arrays
    report.group, report.count, report.rms, report.pair_matched           # per crystal, and per launched pair

Every pair (h, g), h < g, of crystals with equal atom counts is matched with crystal h as the reference side; in
index order a crystal is a representative when it matches no earlier representative, else it joins the earliest
one it matches (the rule of chemeleon_amd.dedup; not transitive).

This is not a port of StructureMatcher, and how far the groups agree with group_structures has not been measured.
Atom counts must be equal: there is no reduction to a primitive cell, so a supercell is never grouped with its
primitive cell (chemeleon_amd.primitive, primitive_states or sample(primitive=...), is the way round it: it runs
first). The pairing is the nearest-partner rule by default; MatchDedup(pairing="assignment") pairs a candidate whose
nearest partners collide by the optimal assignment instead (chemeleon_amd.match; DESIGN.md §4, "Grouping duplicates
by matching" and "Pairing by assignment").
"""

from typing import Optional, Sequence

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd import cell as _cell
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state, exclude_tensor
from chemeleon_amd.match import (COMPOSITION, MANY_ASSIGNMENTS, MANY_MAPPINGS, MATCH_CELL_ANGLE_TOLERANCE,
                                 MATCH_CELL_SYMPREC, MAX_ANGLE_TOL, MAX_ATOMS, MAX_LTOL, MAX_STOL, NO_LATTICE,
                                 PAIR_ASSIGNED_SHIFT, PAIR_FLAG_BITS, PAIRINGS, THIN, check_pairing)

EXCLUDED = 64
FLAG_NAMES = {NO_LATTICE: "no_lattice", COMPOSITION: "composition", THIN: "thin", MANY_MAPPINGS: "many_mappings",
              EXCLUDED: "excluded", MANY_ASSIGNMENTS: "many_assignments"}
RECORD_BYTES = 32
PAIR_RECORD_BYTES = 16


class MatchDedup:
    """When two structures of a batch count as the same crystal: they match within `ltol` (relative length, at most
    1), `stol` (fraction of (V / n)^(1/3), at most 1) and `angle_tol` (degrees, at most 30); the defaults are
    StructureMatcher's; `pairing` is "nearest" or "assignment" (chemeleon_amd.match.Match). Everything is validated
    here, on the host (ValueError)."""

    def __init__(self, ltol: float = 0.2, stol: float = 0.3, angle_tol: float = 5.0, pairing: str = "nearest"):
        self.pairing = check_pairing(pairing)
        for name, v, top in (("ltol", ltol, MAX_LTOL), ("stol", stol, MAX_STOL), ("angle_tol", angle_tol, MAX_ANGLE_TOL)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not 0 < float(np.float32(v)) <= top:
                raise ValueError(f"{name} must be in (0, {top:g}], got {v!r}")
        self.ltol, self.stol, self.angle_tol = float(ltol), float(stol), float(angle_tol)

    def __repr__(self):
        return (f"MatchDedup(ltol={self.ltol}, stol={self.stol}, angle_tol={self.angle_tol}" +
                (f", pairing={self.pairing!r})" if self.pairing != "nearest" else ")"))


def pair_table(natoms: Sequence[int]) -> np.ndarray:
    """The pairs a plan of `natoms` launches, int32 [P, 2] of (h, g): every h < g with equal atom counts, ordered by
    g, then by h (the order of the pair records)."""
    nat = [int(n) for n in natoms]
    earlier, pairs = {}, []
    for g, n in enumerate(nat):
        seen = earlier.setdefault(n, [])
        pairs.extend((h, g) for h in seen)
        seen.append(g)
    return np.array(pairs, dtype=np.int32).reshape(-1, 2)


class MatchGroupReport:
    """One grouping as numpy arrays: group [B] (the representative's index, -1 for an excluded crystal or one
    without a reduced cell), count [B] (the group's size at a representative, else 0), representative [B] bool,
    n_groups; per crystal against its leader rms [B] (units of l; 0 for a leader), max_dist [B] (A), flags [B],
    matched [B] (True for a member), n_assigned [B] (candidates of that pair paired by assignment), ref [B] (the
    leader, -1) and pair [B] (the position of that pair, -1); pair_n_assigned [P] likewise per launched pair;
    `records` the 32-byte records. Per launched pair, in the order of `pairs` [P, 2] = (h, g): pair_rms,
    pair_max_dist, pair_flags, pair_matched, and `pair_records` (16 bytes each). n_searched counts the pairs that
    reached the mapping search."""

    def __init__(self, group, count, records, pair_records, pairs):
        self.group = np.asarray(group, dtype=np.int32)
        self.count = np.asarray(count, dtype=np.int32)
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        f, i = rec.view(np.float32), rec.view(np.int32)
        self.records = rec
        self.rms, self.max_dist = f[:, 0].copy(), f[:, 1].copy()
        self.flags, self.matched, self.ref, self.pair = i[:, 2] & PAIR_FLAG_BITS, i[:, 3] != 0, i[:, 4].copy(), i[:, 5].copy()
        self.n_assigned = i[:, 2] >> PAIR_ASSIGNED_SHIFT
        self.representative = self.group == np.arange(len(self.group), dtype=np.int32)
        self.n_groups = int(self.representative.sum())
        prec = np.ascontiguousarray(pair_records, dtype=np.uint8).reshape(-1, PAIR_RECORD_BYTES)
        pf, pi = prec.view(np.float32), prec.view(np.int32)
        self.pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        self.pair_records = prec
        self.pair_rms, self.pair_max_dist = pf[:, 0].copy(), pf[:, 1].copy()
        self.pair_flags, self.pair_matched = pi[:, 2] & PAIR_FLAG_BITS, pi[:, 3] != 0
        self.pair_n_assigned = pi[:, 2] >> PAIR_ASSIGNED_SHIFT
        self.n_searched = int(((self.pair_flags & ~(MANY_MAPPINGS | MANY_ASSIGNMENTS)) == 0).sum())

    def __len__(self):
        return len(self.group)

    def record(self, g: int) -> dict:
        """What sample() stores in atoms.info["dedup"] for crystal g."""
        return {"index": int(g), "group": int(self.group[g]), "multiplicity": int(self.count[g]),
                "rms": float(self.rms[g])}


class MatchGroupPlan(Plan):
    """Owns a chm_match_group: the node offsets and the pair table of one crystal list on one device."""

    _create, _destroy = "chm_match_group_create", "chm_match_group_destroy"

    def __init__(self, natoms: Sequence[int], device):
        super().__init__(natoms, device)
        lib = _lib.load()
        self.num_pairs = int(lib.chm_match_group_num_pairs(self.handle))
        self.workspace_bytes = int(lib.chm_match_group_workspace_bytes(self.handle))

    def run(self, cell_records, atom_types, frac_coords, lattices, exclude, ltol: float, stol: float, angle_tol: float,
            group, count, out, pair_records, workspace, pairing: str = "nearest"):
        """Enqueues the grouping on the current stream of the plan's device: `cell_records` is the output of
        CellPlan.run on `lattices`, `exclude` None or a uint8 device tensor [B], `group` / `count` int32 [B], `out`
        uint8 of 32 bytes per crystal, `pair_records` uint8 of 16 bytes per pair, `workspace` uint8 of at least
        workspace_bytes. No host wait."""
        _lib.check(_lib.load().chm_match_group_run_pairing(
            self.handle, _lib.ptr(cell_records), cell_records.numel(), _lib.ptr(atom_types), atom_types.numel(),
            _lib.ptr(frac_coords), frac_coords.numel(), _lib.ptr(lattices), lattices.numel(), _lib.ptr(exclude),
            0 if exclude is None else exclude.numel(), float(ltol), float(stol), float(angle_tol), _lib.ptr(group),
            group.numel(), _lib.ptr(count), count.numel(), _lib.ptr(out), out.numel(), _lib.ptr(pair_records),
            pair_records.numel(), _lib.ptr(workspace), workspace.numel(), _lib.stream_handle(self.device),
            PAIRINGS[check_pairing(pairing)]), "chm_match_group_run_pairing")


_plans = PlanCache(MatchGroupPlan)


def match_group_plan(natoms: Sequence[int], device) -> MatchGroupPlan:
    """The plan of this crystal list on this device, cached per (natoms, device) (the last 8)."""
    return _plans.get(device, natoms)


def _need_dedup(dedup) -> MatchDedup:
    if dedup is None:
        return MatchDedup()
    if not isinstance(dedup, MatchDedup):
        raise ValueError("dedup must be a chemeleon_amd.MatchDedup")
    return dedup


def match_group_states(natoms: Sequence[int], atom_types, frac_coords, lattices, dedup: Optional[MatchDedup] = None,
                       exclude=None) -> MatchGroupReport:
    """Groups a state that lives on the device (atom_types [N] int64, frac_coords [N,3] and lattices [B,3,3] fp32,
    in node order of `natoms`; at most 256 atoms per crystal) by pairwise matching and returns its
    MatchGroupReport: the cell pass and the grouping are enqueued on one stream and only the groups and the
    records cross to the host. `exclude` (a bool / 0-1 array or tensor [B]) marks crystals that take no part: they
    get group -1. CPU tensors are refused: there is no host path."""
    dedup = _need_dedup(dedup)
    nat = check_natoms(natoms, MAX_ATOMS, "the matcher")
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices)
    ex = exclude_tensor(exclude, B, "the state lists")
    cells, plan = _cell.cell_plan(nat, dev), match_group_plan(nat, dev)
    with torch.cuda.device(dev):
        if ex is not None:
            ex = ex.to(device=dev, dtype=torch.uint8).contiguous()
        cell_rec = torch.empty(B * _cell.RECORD_BYTES, dtype=torch.uint8, device=dev)
        group = torch.empty(2, B, dtype=torch.int32, device=dev)
        out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
        pair_rec = torch.empty(plan.num_pairs * PAIR_RECORD_BYTES, dtype=torch.uint8, device=dev)
        ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        cells.run(lattices, None, MATCH_CELL_SYMPREC, MATCH_CELL_ANGLE_TOLERANCE, cell_rec)
        plan.run(cell_rec, atom_types, frac_coords, lattices, ex, dedup.ltol, dedup.stol, dedup.angle_tol, group[0],
                 group[1], out, pair_rec, ws, dedup.pairing)
        host = group.cpu().numpy()  # (waits for the kernels; every buffer stays alive until here)
        host_out, host_pairs = out.cpu().numpy(), pair_rec.cpu().numpy()
    return MatchGroupReport(host[0], host[1], host_out, host_pairs, pair_table(nat))
