"""Grouping of duplicate samples on the device: fingerprints and the leader rule.

The reference's workflows go sample -> validity filter -> uniqueness (`test_unique` of scripts/evaluate.py and
the grouping of scripts/navigate_chemical_system.py, both pymatgen's `StructureMatcher().group_structures` on
the host). Here the final state is grouped where it already is (the kernels are csrc/dedup.hip; the fingerprint
and the grouping rule are defined in include/chemeleon_hip.h at chm_dedup_*):

    atoms = model.sample("TiO2", 12, 512, noise="philox", dedup=Dedup())
    model.last_dedup.n_groups        # how many different crystals; `atoms` holds one representative of each
    atoms[0].info["dedup"]           # {"index": its place in the batch, "group": the same, "multiplicity": size}

    report = dedup_states(natoms, a, x, lat, Dedup(tol=0.03))          # device tensors -> numpy arrays
    fps = [fingerprint_states(nat, a, x, lat, d) for ...]              # several cell sizes
    report = group_fingerprints(fps, d)                                # grouped as one list, in list order

This is not a port of StructureMatcher: two crystals are duplicates when their reduced formulas are equal and
their fingerprints (a smooth radial distribution per atom, invariant under permutation, translation, rotation,
change of lattice basis and choice of supercell) differ by at most `tol` relative to the larger norm. How this
criterion agrees with the matcher has not been measured ("Grouping duplicates").
"""

import math
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state, exclude_tensor

DEGENERATE, NONFINITE = 8, 16
CLASSES = 104
MIN_BINS, MAX_BINS = 8, 256


class Dedup:
    """When two structures count as the same crystal: equal reduced formulas and fingerprints within `tol`
    (relative to the larger norm). `r_cut` (A), `sigma` (A) and `bins` (per channel) define the fingerprint.
    The default tol is a design choice, not a measurement. Everything is validated here, on the host
    (ValueError)."""

    def __init__(self, tol: float = 0.05, r_cut: float = 6.0, sigma: float = 0.15, bins: int = 64):
        for name, v in (("tol", tol), ("r_cut", r_cut), ("sigma", sigma)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not (float(v) > 0 and math.isfinite(float(v))):
                raise ValueError(f"{name} must be positive and finite, got {v!r}")
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not MIN_BINS <= int(bins) <= MAX_BINS:
            raise ValueError(f"bins must be an integer in [{MIN_BINS}, {MAX_BINS}], got {bins!r}")
        self.tol, self.r_cut, self.sigma, self.bins = float(tol), float(r_cut), float(sigma), int(bins)

    def __repr__(self):
        return f"Dedup(tol={self.tol}, r_cut={self.r_cut}, sigma={self.sigma}, bins={self.bins})"


class Fingerprints:
    """The fingerprints of one crystal list as device tensors: fp [B, 2 * bins] float32, counts [B, 104] int32
    (reduced element counts) and flags [B] int32 (DEGENERATE, NONFINITE; 0 = usable)."""

    def __init__(self, fp, counts, flags):
        self.fp, self.counts, self.flags = fp, counts, flags

    @property
    def bins(self) -> int:
        return self.fp.shape[1] // 2

    def __len__(self):
        return self.fp.shape[0]


class DedupReport:
    """One grouping as numpy arrays: group [B] (the representative's index, -1 for a flagged or excluded
    crystal), count [B] (the group's size at a representative, else 0), representative [B] bool, flags [B]
    (the fingerprints' flags) and n_groups."""

    def __init__(self, group: np.ndarray, count: np.ndarray, flags: np.ndarray):
        self.group = np.asarray(group, dtype=np.int32)
        self.count = np.asarray(count, dtype=np.int32)
        self.flags = np.asarray(flags, dtype=np.int32)
        self.representative = self.group == np.arange(len(self.group), dtype=np.int32)
        self.n_groups = int(self.representative.sum())

    def __len__(self):
        return len(self.group)

    def record(self, g: int) -> dict:
        """What sample() stores in atoms.info["dedup"] for crystal g."""
        return {"index": int(g), "group": int(self.group[g]), "multiplicity": int(self.count[g])}


class DedupPlan(Plan):
    """Owns a chm_dedup: the node offsets of one crystal list on one device."""

    _create, _destroy = "chm_dedup_create", "chm_dedup_destroy"

    def fingerprint(self, atom_types, frac_coords, lattices, dedup: Dedup, fp, counts, flags):
        """Enqueues the fingerprint kernel on the current stream of the plan's device. No host wait."""
        _lib.check(_lib.load().chm_dedup_fingerprint(
            self.handle, _lib.ptr(atom_types), atom_types.numel(), _lib.ptr(frac_coords), frac_coords.numel(),
            _lib.ptr(lattices), lattices.numel(), dedup.bins, dedup.r_cut, dedup.sigma, _lib.ptr(fp), fp.numel(),
            _lib.ptr(counts), counts.numel(), _lib.ptr(flags), flags.numel(), _lib.stream_handle(self.device)),
            "chm_dedup_fingerprint")


_plans = PlanCache(DedupPlan)


def dedup_plan(natoms: Sequence[int], device) -> DedupPlan:
    """The plan of this crystal list on this device, cached per (natoms, device) (the last 8)."""
    return _plans.get(device, natoms)


def _need_dedup(dedup) -> Dedup:
    if dedup is None:
        return Dedup()
    if not isinstance(dedup, Dedup):
        raise ValueError("dedup must be a chemeleon_amd.Dedup")
    return dedup


def fingerprint_states(natoms: Sequence[int], atom_types, frac_coords, lattices, dedup: Optional[Dedup] = None
                       ) -> Fingerprints:
    """The fingerprints of a state that lives on the device (atom_types [N] int64, frac_coords [N,3] and
    lattices [B,3,3] fp32, in node order of `natoms`), left on the device. CPU tensors are refused: there is no
    host path. No host wait."""
    dedup = _need_dedup(dedup)
    nat = check_natoms(natoms)
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices)
    plan = dedup_plan(nat, dev)
    with torch.cuda.device(dev):
        fp = torch.empty(B, 2 * dedup.bins, dtype=torch.float32, device=dev)
        counts = torch.empty(B, CLASSES, dtype=torch.int32, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        plan.fingerprint(atom_types, frac_coords, lattices, dedup, fp, counts, flags)
    return Fingerprints(fp, counts, flags)


def group_on_device(fps: Fingerprints, tol: float, exclude=None):
    """Enqueues the grouping of one Fingerprints on the current stream -> (group, count) int32 device tensors
    (and the workspace is kept alive by the caching allocator's stream order). `exclude`: a uint8 / bool device
    tensor [B] or None. No host wait."""
    B, dev = len(fps), fps.fp.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        group = torch.empty(B, dtype=torch.int32, device=dev)
        count = torch.empty(B, dtype=torch.int32, device=dev)
        nbytes = lib.chm_dedup_workspace_bytes(B)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.chm_dedup_group(
            B, fps.bins, _lib.ptr(fps.fp), fps.fp.numel(), _lib.ptr(fps.counts), fps.counts.numel(),
            _lib.ptr(fps.flags), fps.flags.numel(), _lib.ptr(exclude), 0 if exclude is None else exclude.numel(),
            float(tol), _lib.ptr(group), group.numel(), _lib.ptr(count), count.numel(), _lib.ptr(ws), nbytes,
            _lib.stream_handle(dev)), "chm_dedup_group")
    return group, count


def group_fingerprints(fps: Union[Fingerprints, Sequence[Fingerprints]], dedup: Optional[Dedup] = None,
                       exclude=None) -> DedupReport:
    """Groups fingerprints by the leader rule: in index order a crystal is a representative when it matches no
    earlier representative, otherwise it joins the earliest one it matches. `fps` is one Fingerprints or a list
    of them (concatenated on the device, in list order: the union over several cell sizes groups as one list).
    `exclude` (a bool / 0-1 array or tensor of the total length) marks crystals that take no part: they and the
    flagged ones get group -1. Only group, count and flags cross to the host."""
    dedup = _need_dedup(dedup)
    many = [fps] if isinstance(fps, Fingerprints) else list(fps)
    if not many or not all(isinstance(f, Fingerprints) for f in many):
        raise ValueError("fps must be a Fingerprints or a non-empty list of them")
    for f in many:
        if f.fp.dim() != 2 or f.fp.shape[1] != 2 * dedup.bins:
            raise ValueError(f"fingerprints of {f.fp.shape[-1] // 2} bins, the Dedup has {dedup.bins}")
        if tuple(f.counts.shape) != (len(f), CLASSES) or tuple(f.flags.shape) != (len(f),):
            raise ValueError("counts must be [B,104] and flags [B] for fp [B,2*bins]")
        if f.fp.dtype != torch.float32 or f.counts.dtype != torch.int32 or f.flags.dtype != torch.int32:
            raise ValueError("fingerprints must be fp float32, counts / flags int32")
    B = sum(len(f) for f in many)
    if B < 1:
        raise ValueError("no fingerprints to group")
    ex = exclude_tensor(exclude, B, "the fingerprints list")
    for f in many:
        _lib.require_device(f.fp, f.counts, f.flags)
    dev = many[0].fp.device
    if any(t.device != dev for f in many for t in (f.fp, f.counts, f.flags)):
        raise ValueError("the fingerprints are on different devices")
    with torch.cuda.device(dev):
        one = many[0] if len(many) == 1 else Fingerprints(
            torch.cat([f.fp for f in many]), torch.cat([f.counts for f in many]), torch.cat([f.flags for f in many]))
        if ex is not None:
            ex = ex.to(device=dev, dtype=torch.uint8).contiguous()
        group, count = group_on_device(one, dedup.tol, ex)
        host = torch.stack([group, count, one.flags]).cpu().numpy()  # (waits for the grouping)
    return DedupReport(host[0], host[1], host[2])


def dedup_states(natoms: Sequence[int], atom_types, frac_coords, lattices, dedup: Optional[Dedup] = None,
                 exclude=None) -> DedupReport:
    """fingerprint_states, then group_fingerprints, of one state on the device."""
    dedup = _need_dedup(dedup)
    return group_fingerprints(fingerprint_states(natoms, atom_types, frac_coords, lattices, dedup), dedup, exclude)


def deduped_atoms(natoms: Sequence[int], atom_types, frac_coords, lattices, dedup: Dedup, screen=None):
    """(representatives, DedupReport, ScreenReport or None): groups the state on the device (after the screen,
    whose failures are excluded) and copies and converts only the representatives, each with
    atoms.info["dedup"] (and info["screen"] with a screen)."""
    from chemeleon_amd.finish import finish_atoms
    atoms, reports = finish_atoms(natoms, atom_types, frac_coords, lattices, screen=screen, dedup=_need_dedup(dedup))
    return atoms, reports["dedup"], reports.get("screen")
