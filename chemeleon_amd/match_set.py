"""Searching a set of reference structures for each sampled structure on the device: known or novel.

The users of the reference's scripts/navigate_chemical_system.py first strike out of its output what is already
known (the training set, or an earlier run's representatives); its own last step merges each composition's unique
structures into one list. Both ask of every sample: is it any structure of a given set? Here the whole set is
searched where the final state already is (the kernels are csrc/match.hip; the definition is in
include/chemeleon_hip.h at chm_match_set_*):

    known = ReferenceSet.from_atoms(training_structures)              # sorted on the host, on the device once
    atoms = model.sample("Ti-O", 12, 512, noise="philox", screen=Screen(...),
                         search=MatchSet(known, require="novel"), dedup=MatchDedup())   # valid, novel, unique
    model.last_search.novelty_rate
    atoms[0].info["search"]                                           # {"known", "ref", "rms", ...}

    report = match_set_states(natoms, a, x, lat, MatchSet(known))     # device tensors -> numpy arrays
    report.known, report.ref, report.candidates(g)

Every structure has a composition key (a 64-bit sum over its atoms that does not depend on their order); the set is
held sorted by (atom count, key, original index), so the candidates of a sample, the references with its atom count
and its composition, are one range that the device finds by binary search from the atom types it sampled. Each
candidate is one match under the definition of chemeleon_amd.match with `ltol` / `stol` / `angle_tol`, the
reference being the reference side; a sample is known when a candidate matches, and `ref` is the matched
candidate with the smallest rms (ties: the smallest original index).

This is not a port of StructureMatcher, and how far known / novel agree with StructureMatcher.fit against every
structure of the set has not been measured. Atom counts must be equal: there is no reduction to a primitive cell,
so a supercell is never found to be its primitive cell (chemeleon_amd.primitive, primitive_states or
sample(primitive=...), is the way round it: it runs first; reduce the set likewise). The pairing is the
nearest-partner rule by default; MatchSet(..., pairing="assignment") pairs a candidate whose nearest partners collide
by the optimal assignment instead (chemeleon_amd.match; DESIGN.md §4, "Searching a reference set" and "Pairing by
assignment").
"""

import itertools
import weakref
from typing import Optional, Sequence

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd import cell as _cell
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state, exclude_tensor, int32_array
from chemeleon_amd.match import (COMPOSITION, MANY_MAPPINGS, MATCH_CELL_ANGLE_TOLERANCE, MATCH_CELL_SYMPREC, MAX_ANGLE_TOL,
                                 MAX_ATOMS, MAX_LTOL, MAX_STOL, NO_LATTICE, PAIR_ASSIGNED_SHIFT, PAIR_FLAG_BITS, PAIRINGS,
                                 THIN, Reference, check_pairing)
from chemeleon_amd.match_group import EXCLUDED, FLAG_NAMES, PAIR_RECORD_BYTES

RECORD_BYTES = 48
MIX_A, MIX_B = np.uint64(0xbf58476d1ce4e5b9), np.uint64(0x94d049bb133111eb)


def composition_keys(natoms: Sequence[int], atom_types) -> np.ndarray:
    """uint64 [len(natoms)]: per structure the wrapping sum over its atoms of the splitmix64 finaliser of t + 1, t the
    atom type's low 32 bits (include/chemeleon_hip.h at chm_match_set_*)."""
    t = np.asarray(atom_types).astype(np.int64)
    with np.errstate(over="ignore"):
        z = (t & 0xffffffff).astype(np.uint64) + np.uint64(1)
        z = (z ^ (z >> np.uint64(30))) * MIX_A
        z = (z ^ (z >> np.uint64(27))) * MIX_B
        z = z ^ (z >> np.uint64(31))
        first = np.concatenate([[0], np.cumsum(natoms)[:-1]]).astype(np.int64)
        return np.add.reduceat(z, first).astype(np.uint64)


_tokens = itertools.count(1)
_sets = weakref.WeakValueDictionary()  # token -> ReferenceSet: what a plan's cache key stands for


class ReferenceSet:
    """R reference structures to search, given like a Reference (natoms [R], atom_types [NR], frac_coords [NR,3],
    lattices [R,3,3]; validated the same way) and held sorted by (atom count, composition key, original index):
    `order` [R] is the original index of each sorted position, `keys` [R] the sorted keys, `natoms`, `atom_types`,
    `frac_coords`, `lattices` the sorted structures. They go to a device, with their cell records, once per device."""

    def __init__(self, natoms, atom_types, frac_coords, lattices):
        given = Reference(natoms, atom_types, frac_coords, lattices)
        nat = np.array(given.natoms, dtype=np.int64)
        keys = composition_keys(nat, given.atom_types)
        order = np.lexsort((np.arange(len(nat)), keys, nat))
        first = np.concatenate([[0], np.cumsum(nat)[:-1]])
        nodes = np.concatenate([np.arange(first[r], first[r] + nat[r]) for r in order])
        self.order = order.astype(np.int32)
        self.keys = np.ascontiguousarray(keys[order])
        self.sorted = Reference(nat[order].tolist(), given.atom_types[nodes], given.frac_coords[nodes],
                                given.lattices[order])
        self.natoms, self.atom_types = self.sorted.natoms, self.sorted.atom_types
        self.frac_coords, self.lattices = self.sorted.frac_coords, self.sorted.lattices
        self.token = next(_tokens)
        _sets[self.token] = self

    @classmethod
    def from_arrays(cls, natoms, atom_types, frac_coords, lattices) -> "ReferenceSet":
        return cls(natoms, atom_types, frac_coords, lattices)

    @classmethod
    def from_atoms(cls, atoms) -> "ReferenceSet":
        """From one ase.Atoms or a list of them (atomic numbers, scaled positions, cell)."""
        given = Reference.from_atoms(atoms)
        return cls(given.natoms, given.atom_types, given.frac_coords, given.lattices)

    def __len__(self):
        return len(self.natoms)

    def on(self, device):
        """(atom_types, frac_coords, lattices, cell records) of the sorted set on `device`, made once per device."""
        return self.sorted.on(device)


class MatchSet:
    """How finished structures are searched for in `reference_set` (a ReferenceSet): the tolerances `ltol` (relative
    length, at most 1), `stol` (fraction of (V / n)^(1/3), at most 1) and `angle_tol` (degrees, at most 30) of each
    match, and `require`: with "known" the structures that are in no way in the set count as failed in sample() /
    finish_atoms, with "novel" the ones that are; `pairing` is "nearest" or "assignment" (chemeleon_amd.match.Match).
    Everything is validated here, on the host (ValueError)."""

    def __init__(self, reference_set: ReferenceSet, ltol: float = 0.2, stol: float = 0.3, angle_tol: float = 5.0,
                 require: Optional[str] = None, pairing: str = "nearest"):
        self.pairing = check_pairing(pairing)
        if not isinstance(reference_set, ReferenceSet):
            raise ValueError("reference_set must be a chemeleon_amd.ReferenceSet")
        for name, v, top in (("ltol", ltol, MAX_LTOL), ("stol", stol, MAX_STOL), ("angle_tol", angle_tol, MAX_ANGLE_TOL)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not 0 < float(np.float32(v)) <= top:
                raise ValueError(f"{name} must be in (0, {top:g}], got {v!r}")
        if require not in (None, "known", "novel"):
            raise ValueError(f"require must be None, 'known' or 'novel', got {require!r}")
        self.reference_set = reference_set
        self.ltol, self.stol, self.angle_tol, self.require = float(ltol), float(stol), float(angle_tol), require

    def __repr__(self):
        return (f"MatchSet({len(self.reference_set)} references, ltol={self.ltol}, stol={self.stol}, "
                f"angle_tol={self.angle_tol}, require={self.require!r}" +
                (f", pairing={self.pairing!r})" if self.pairing != "nearest" else ")"))


class MatchSetReport:
    """One search as numpy arrays, per sample: known [B] and novel [B] (bool; an excluded sample or one without a
    reduced cell is neither), ref [B] (the winner's original index, -1), position [B] (its sorted position, -1), rms
    [B] (units of l of that reference), max_dist [B] (A), n_assigned [B] (candidates of the winner's pair paired by
    assignment; pair_n_assigned per launched pair), n_candidates [B], n_matched [B], key [B] (uint64), flags
    [B], first [B] and lo [B] (where the sample's pair records and its candidates start); n_known, n_novel,
    novelty_rate (novel over the samples that were searched; nan if none), mismatch [B] according to `require`
    (all False without one); `records` the 48-byte records. Per launched pair, in the order of the samples and of
    the sorted set: pair_sample, pair_ref (original index), pair_rms, pair_max_dist, pair_flags, pair_matched, and
    `pair_records` (16 bytes each)."""

    def __init__(self, records, pair_records, order, require: Optional[str] = None):
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        f, i = rec.view(np.float32), rec.view(np.int32)
        self.records = rec
        self.rms, self.max_dist = f[:, 0].copy(), f[:, 1].copy()
        self.flags, self.known = i[:, 2] & PAIR_FLAG_BITS, i[:, 3] != 0
        self.n_assigned = i[:, 2] >> PAIR_ASSIGNED_SHIFT
        self.ref, self.position = i[:, 4].copy(), i[:, 5].copy()
        self.n_candidates, self.n_matched = i[:, 6].copy(), i[:, 7].copy()
        self.key = rec.view(np.uint64)[:, 4].copy()
        self.first, self.lo = i[:, 10].copy(), i[:, 11].copy()
        self.searched = (self.flags & (EXCLUDED | NO_LATTICE)) == 0
        self.novel = self.searched & ~self.known
        self.n_known, self.n_novel = int(self.known.sum()), int(self.novel.sum())
        n = int(self.searched.sum())
        self.novelty_rate = self.n_novel / n if n else float("nan")
        self.require = require
        self.mismatch = ~self.known if require == "known" else ~self.novel if require == "novel" else \
            np.zeros(len(rec), dtype=bool)
        P = int(self.n_candidates.sum())
        prec = np.ascontiguousarray(pair_records, dtype=np.uint8).reshape(-1, PAIR_RECORD_BYTES)[:P]
        pf, pi = prec.view(np.float32), prec.view(np.int32)
        self.order = np.asarray(order, dtype=np.int32)
        self.pair_records = prec
        self.pair_sample = np.repeat(np.arange(len(rec), dtype=np.int32), self.n_candidates)
        within = np.arange(P, dtype=np.int64) - np.repeat(self.first.astype(np.int64), self.n_candidates)
        self.pair_ref = self.order[np.repeat(self.lo.astype(np.int64), self.n_candidates) + within] if P else \
            np.zeros(0, dtype=np.int32)
        self.pair_rms, self.pair_max_dist = pf[:, 0].copy(), pf[:, 1].copy()
        self.pair_flags, self.pair_matched = pi[:, 2] & PAIR_FLAG_BITS, pi[:, 3] != 0
        self.pair_n_assigned = pi[:, 2] >> PAIR_ASSIGNED_SHIFT

    def __len__(self):
        return len(self.flags)

    def candidates(self, g: int):
        """(original indices, matched, rms) of sample g's candidates, in the sorted set's order."""
        s = slice(int(self.first[g]), int(self.first[g]) + int(self.n_candidates[g]))
        return self.pair_ref[s].copy(), self.pair_matched[s].copy(), self.pair_rms[s].copy()

    def record(self, g: int) -> dict:
        """Sample g's record as a dict of Python numbers (what sample() stores in atoms.info["search"])."""
        fl = int(self.flags[g])
        return {"known": bool(self.known[g]), "novel": bool(self.novel[g]), "ref": int(self.ref[g]),
                "rms": float(self.rms[g]), "max_dist": float(self.max_dist[g]), "n_candidates": int(self.n_candidates[g]),
                "n_matched": int(self.n_matched[g]), "n_assigned": int(self.n_assigned[g]), "key": int(self.key[g]),
                "flags": fl,
                "failed": [name for bit, name in FLAG_NAMES.items() if fl & bit]}


class MatchSetPlan(Plan):
    """Owns a chm_match_set: the node offsets of a crystal list and of a sorted reference set, its keys and indices,
    on one device."""

    _create, _destroy = "chm_match_set_create", "chm_match_set_destroy"

    def __init__(self, natoms: Sequence[int], reference_set: ReferenceSet, device):
        self.natoms = tuple(int(n) for n in natoms)
        self.reference_set = reference_set
        self.device = torch.device(device)
        R = len(reference_set)
        keys = (_lib.c_u64 * R).from_buffer_copy(reference_set.keys.tobytes())
        self._make(int32_array(self.natoms), len(self.natoms), int32_array(reference_set.natoms), keys,
                   int32_array(reference_set.order.tolist()), R)
        lib = _lib.load()
        self.num_pairs_max = int(lib.chm_match_set_num_pairs_max(self.handle))
        self.workspace_bytes = int(lib.chm_match_set_workspace_bytes(self.handle))

    def run(self, cell_records, atom_types, frac_coords, lattices, ref_cell_records, ref_atom_types, ref_frac_coords,
            ref_lattices, exclude, ltol: float, stol: float, angle_tol: float, out, pair_records, workspace,
            pairing: str = "nearest"):
        """Enqueues the search on the current stream of the plan's device: the cell records are the outputs of
        CellPlan.run on the two lattice lists (the references in sorted order), `exclude` None or a uint8 device
        tensor [B], `out` uint8 of 48 bytes per crystal, `pair_records` uint8 of 16 bytes x num_pairs_max (None when
        that is 0), `workspace` uint8 of at least workspace_bytes. No host wait."""
        _lib.check(_lib.load().chm_match_set_run_pairing(
            self.handle, _lib.ptr(cell_records), cell_records.numel(), _lib.ptr(atom_types), atom_types.numel(),
            _lib.ptr(frac_coords), frac_coords.numel(), _lib.ptr(lattices), lattices.numel(),
            _lib.ptr(ref_cell_records), ref_cell_records.numel(), _lib.ptr(ref_atom_types), ref_atom_types.numel(),
            _lib.ptr(ref_frac_coords), ref_frac_coords.numel(), _lib.ptr(ref_lattices), ref_lattices.numel(),
            _lib.ptr(exclude), 0 if exclude is None else exclude.numel(), float(ltol), float(stol), float(angle_tol),
            _lib.ptr(out), out.numel(), _lib.ptr(pair_records), 0 if pair_records is None else pair_records.numel(),
            _lib.ptr(workspace), workspace.numel(), _lib.stream_handle(self.device), PAIRINGS[check_pairing(pairing)]),
            "chm_match_set_run_pairing")


_plans = PlanCache(lambda natoms, token, device: MatchSetPlan(natoms, _sets[token[0]], device))


def match_set_plan(natoms: Sequence[int], reference_set: ReferenceSet, device) -> MatchSetPlan:
    """The plan of this crystal list and this set on this device, cached per (natoms, set, device) (the last 8)."""
    return _plans.get(device, natoms, (reference_set.token,))


def match_set_states(natoms: Sequence[int], atom_types, frac_coords, lattices, match_set: MatchSet,
                     exclude=None) -> MatchSetReport:
    """Searches match_set.reference_set for every crystal of a state that lives on the device (atom_types [N] int64,
    frac_coords [N,3] and lattices [B,3,3] fp32, in node order of `natoms`; at most 256 atoms per crystal) and
    returns its MatchSetReport: the cell pass and the search are enqueued on one stream and only the records cross
    to the host. `exclude` (a bool / 0-1 array or tensor [B]) marks crystals that are not searched. CPU tensors are
    refused: there is no host path."""
    if not isinstance(match_set, MatchSet):
        raise ValueError("search must be a chemeleon_amd.MatchSet")
    nat = check_natoms(natoms, MAX_ATOMS, "the matcher")
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices)
    ex = exclude_tensor(exclude, B, "the state lists")
    rs = match_set.reference_set
    ra, rx, rlat, rrec = rs.on(dev)
    cells, plan = _cell.cell_plan(nat, dev), match_set_plan(nat, rs, dev)
    with torch.cuda.device(dev):
        if ex is not None:
            ex = ex.to(device=dev, dtype=torch.uint8).contiguous()
        cell_rec = torch.empty(B * _cell.RECORD_BYTES, dtype=torch.uint8, device=dev)
        out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
        cap = plan.num_pairs_max
        pair_rec = torch.empty(cap * PAIR_RECORD_BYTES, dtype=torch.uint8, device=dev) if cap else None
        ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
        cells.run(lattices, None, MATCH_CELL_SYMPREC, MATCH_CELL_ANGLE_TOLERANCE, cell_rec)
        plan.run(cell_rec, atom_types, frac_coords, lattices, rrec, ra, rx, rlat, ex, match_set.ltol, match_set.stol,
                 match_set.angle_tol, out, pair_rec, ws, match_set.pairing)
        host = out.cpu().numpy()  # (waits for the kernels; every buffer stays alive until here)
        P = int(host.view(np.int32).reshape(B, -1)[:, 6].sum())
        host_pairs = pair_rec[:P * PAIR_RECORD_BYTES].cpu().numpy() if P else np.zeros(0, dtype=np.uint8)
    return MatchSetReport(host, host_pairs, rs.order, match_set.require)
