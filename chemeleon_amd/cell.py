"""Lattice system and reduced cell of sampled structures on the device.

The reference's scripts/evaluate.py asks pymatgen / spglib on the host which lattice system a generated cell has
(`test_lattice_system_matching`: the atoms are replaced by one H, so it is a question about the lattice alone),
and its models take the crystal system as a text target. Here the final state is classified where it already
is (the kernels are csrc/cell.hip; the definition is in include/chemeleon_hip.h at chm_cell_*):

    atoms = model.sample("cubic", 8, 512, noise="philox", cell=Cell(require="cubic", reduce=True))
    model.last_cell.system           # [512] names: what every sample came out as; `atoms` holds the cubic ones
    atoms[0].info["cell"]            # the structure's record as a dict; its cell is the Niggli-reduced one

    report = cell_states(natoms, a, x, lat, Cell(symprec=0.05))          # device tensors -> numpy arrays
    x_r, lat_r, report = reduce_states(natoms, a, x, lat)                # the state in its reduced cells, on device

Per crystal: Niggli reduction (Lr = T L, T integer with det +1), then the search of every integer matrix W with
entries in {-1, 0, 1} and |det W| = 1 that maps Lr onto itself within `symprec` (A, row lengths) and
`angle_tolerance` (degrees, inter-row angles); the set's size and its rotation orders name the holohedry. A set
that is no group halves both tolerances, at most four times. This is not a port of spglib: how far the two agree
on real samples has not been measured; the crystal system with the atoms is chemeleon_amd.symmetry
("Lattice system and reduced cell").
"""

from typing import Optional, Sequence, Union

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state

SYSTEMS = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "rhombohedral", "hexagonal", "cubic")
AMBIGUOUS, MISMATCH, NOT_REDUCED, DEGENERATE, NONFINITE = 1, 2, 4, 8, 16
FLAG_NAMES = {AMBIGUOUS: "ambiguous", MISMATCH: "mismatch", NOT_REDUCED: "not_reduced", DEGENERATE: "degenerate",
              NONFINITE: "nonfinite"}
RECORD_BYTES = 128
MAX_SYMPREC, MAX_ANGLE_TOLERANCE = 1.0, 30.0


def system_code(name) -> int:
    """"cubic" -> 6; ValueError for anything that is not one of SYSTEMS."""
    if not isinstance(name, str) or name not in SYSTEMS:
        raise ValueError(f"unknown lattice system {name!r}: expected one of {', '.join(SYSTEMS)}")
    return SYSTEMS.index(name)


class Cell:
    """How a finished structure's lattice is classified: `symprec` (A, at most 1) and `angle_tolerance` (degrees,
    at most 30) are the tolerances of the search (the defaults are the reference's). `require` names the lattice
    system a structure must have (one name for every crystal, or a list with one name per crystal; a cell
    without a system, flagged or not reduced, never meets it); `reduce` asks for the structures in their
    Niggli-reduced cells. Everything is validated here, on the host
    (ValueError)."""

    def __init__(self, symprec: float = 0.1, angle_tolerance: float = 10.0,
                 require: Optional[Union[str, Sequence[str]]] = None, reduce: bool = False):
        for name, v, top in (("symprec", symprec, MAX_SYMPREC), ("angle_tolerance", angle_tolerance, MAX_ANGLE_TOLERANCE)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not 0 < float(np.float32(v)) <= top:
                raise ValueError(f"{name} must be in (0, {top:g}], got {v!r}")
        if not isinstance(reduce, (bool, np.bool_)):
            raise ValueError(f"reduce must be a bool, got {reduce!r}")
        self.symprec, self.angle_tolerance, self.reduce = float(symprec), float(angle_tolerance), bool(reduce)
        self.require = require
        if require is None:
            self.codes = None
        elif isinstance(require, str):
            self.codes = np.array([system_code(require)], dtype=np.int32)
        else:
            try:
                names = list(require)
            except TypeError:
                raise ValueError(f"require must be a lattice system's name or a list of them, got {require!r}") from None
            if not names:
                raise ValueError("require: an empty list of lattice systems")
            self.codes = np.array([system_code(n) for n in names], dtype=np.int32)
        self._per_crystal = require is not None and not isinstance(require, str)

    def codes_for(self, num_graphs: int) -> Optional[np.ndarray]:
        """The int32 required codes of a batch of num_graphs crystals ([1], [num_graphs] or None); ValueError if
        a per-crystal list has another length."""
        if self._per_crystal and len(self.codes) != num_graphs:
            raise ValueError(f"require lists {len(self.codes)} lattice systems, the batch has {num_graphs} crystals")
        return self.codes

    def __repr__(self):
        return (f"Cell(symprec={self.symprec}, angle_tolerance={self.angle_tolerance}, require={self.require!r}, "
                f"reduce={self.reduce})")


class CellReport:
    """The records of one batch as numpy arrays: system [B] (names; "" where none), code [B] (-1 where none),
    lengths [B,3], angles [B,3] (alpha, beta, gamma in degrees) and volume [B] of the reduced cell, transform
    [B,3,3] (T: reduced = T @ lattice), n_ops [B], orders [B,4] (n2, n3, n4, n6), halvings [B], passes [B], flags
    [B], mismatch [B] (a required system was not met) and valid [B] (flags == 0: a system was found and no
    requirement failed; a cell the reduction did not finish has no system)."""

    def __init__(self, records: np.ndarray):
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        f = rec.view(np.float32)
        i = rec.view(np.int32)
        self.records = rec
        self.lengths = f[:, 0:3].copy()
        self.angles = f[:, 3:6].copy()
        self.volume = f[:, 6].copy()
        self.transform = i[:, 8:17].reshape(-1, 3, 3).copy()
        self.n_ops = i[:, 17].copy()
        self.orders = i[:, 18:22].copy()
        self.code = i[:, 22].copy()
        self.halvings = i[:, 23].copy()
        self.flags = i[:, 24].copy()
        self.passes = i[:, 25].copy()
        self.system = np.array([SYSTEMS[c] if 0 <= c < len(SYSTEMS) else "" for c in self.code])
        self.mismatch = (self.flags & MISMATCH) != 0
        self.valid = (self.flags == 0) & (self.code >= 0)

    def __len__(self):
        return len(self.flags)

    def record(self, g: int) -> dict:
        """Crystal g's record as a dict of Python numbers (what sample() stores in atoms.info["cell"])."""
        fl = int(self.flags[g])
        return {"system": str(self.system[g]) or None, "code": int(self.code[g]),
                "lengths": tuple(float(v) for v in self.lengths[g]), "angles": tuple(float(v) for v in self.angles[g]),
                "volume": float(self.volume[g]), "transform": tuple(tuple(int(v) for v in r) for r in self.transform[g]),
                "n_ops": int(self.n_ops[g]), "orders": tuple(int(v) for v in self.orders[g]),
                "halvings": int(self.halvings[g]), "flags": fl,
                "failed": [name for bit, name in FLAG_NAMES.items() if fl & bit], "valid": bool(self.valid[g])}


class CellPlan(Plan):
    """Owns a chm_cell: the node offsets of one crystal list on one device."""

    _create, _destroy = "chm_cell_create", "chm_cell_destroy"

    def run(self, lattices, require, symprec: float, angle_tolerance: float, out):
        """Enqueues the classification on the current stream of the plan's device; `out` is a uint8 device tensor
        of 128 bytes per crystal, `require` an int32 device tensor or None. No host wait."""
        _lib.check(_lib.load().chm_cell_run(
            self.handle, _lib.ptr(lattices), lattices.numel(), _lib.ptr(require),
            0 if require is None else require.numel(), float(symprec), float(angle_tolerance), _lib.ptr(out),
            out.numel(), _lib.stream_handle(self.device)), "chm_cell_run")
        return out

    def apply(self, records, frac_coords, lattices, frac_out, lattices_out):
        """Enqueues the change to the reduced cells of `records` (a run's output) into frac_out / lattices_out,
        which must not be the inputs. No host wait."""
        _lib.check(_lib.load().chm_cell_apply(
            self.handle, _lib.ptr(records), records.numel(), _lib.ptr(frac_coords), frac_coords.numel(),
            _lib.ptr(lattices), lattices.numel(), _lib.ptr(frac_out), frac_out.numel(), _lib.ptr(lattices_out),
            lattices_out.numel(), _lib.stream_handle(self.device)), "chm_cell_apply")
        return frac_out, lattices_out


_plans = PlanCache(CellPlan)


def cell_plan(natoms: Sequence[int], device) -> CellPlan:
    """The plan of this crystal list on this device, cached per (natoms, device) (the last 8)."""
    return _plans.get(device, natoms)


def _need_cell(cell) -> Cell:
    if cell is None:
        return Cell()
    if not isinstance(cell, Cell):
        raise ValueError("cell must be a chemeleon_amd.Cell")
    return cell


def _run(natoms, atom_types, frac_coords, lattices, cell, reduce):
    cell = _need_cell(cell)
    nat = check_natoms(natoms)
    codes = cell.codes_for(len(nat))
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices, types_used=False)
    plan = cell_plan(nat, dev)
    x_out = lat_out = None
    with torch.cuda.device(dev):
        rq = None if codes is None else torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
        out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
        plan.run(lattices, rq, cell.symprec, cell.angle_tolerance, out)
        if reduce:
            x_out, lat_out = torch.empty_like(frac_coords), torch.empty_like(lattices)
            plan.apply(out, frac_coords, lattices, x_out, lat_out)
        host = out.cpu().numpy()  # (waits for the kernels; rq and out stay alive until here)
    return x_out, lat_out, CellReport(host)


def cell_states(natoms: Sequence[int], atom_types, frac_coords, lattices, cell: Optional[Cell] = None) -> CellReport:
    """Classifies the lattices of a state that lives on the device (frac_coords [N,3] and lattices [B,3,3] fp32,
    in node order of `natoms`; atom_types [N] takes no part and may be None) and returns its CellReport; only
    the 128-byte records cross to the host. CPU tensors are refused: there is no host path."""
    return _run(natoms, atom_types, frac_coords, lattices, cell, False)[2]


def reduce_states(natoms: Sequence[int], atom_types, frac_coords, lattices, cell: Optional[Cell] = None):
    """(frac_coords, lattices, report): the state in its Niggli-reduced cells as new device tensors (the
    coordinates in [0, 1); the inputs are not changed) and the CellReport of the same run."""
    return _run(natoms, atom_types, frac_coords, lattices, cell, True)


def finished_atoms(natoms: Sequence[int], atom_types, frac_coords, lattices, cell: Cell, screen=None, dedup=None):
    """(structures, CellReport, ScreenReport or None, DedupReport or None): the tail of sample() with cell=. The
    screen runs first, then the cell, then the grouping, from which the failures of both (a screen flag; a
    required system not met) are excluded. Only the structures that pass are copied and converted (in their
    reduced cells with cell.reduce), each with atoms.info["cell"] (and info["screen"] / info["dedup"])."""
    from chemeleon_amd.finish import finish_atoms
    atoms, reports = finish_atoms(natoms, atom_types, frac_coords, lattices, screen=screen, cell=_need_cell(cell), dedup=dedup)
    return atoms, reports["cell"], reports.get("screen"), reports.get("dedup")
