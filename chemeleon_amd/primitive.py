"""Primitive cells of sampled structures on the device.

A diffusion sampler asked for 8 atoms of a 2-atom compound returns supercells routinely (the reference's
navigate_chemical_system.py samples one reduced formula at n_atoms = reduced_natoms * f for f = 1..13 and expects
group_structures to merge the results). The symmetry, matching and grouping legs describe the cell as given; this
leg gives them primitive cells (the kernels are csrc/prim.hip; the definition is in include/chemeleon_hip.h at
chm_prim_*):

    atoms = model.sample("NaCl", 8, 512, noise="philox", primitive=Primitive(), dedup=MatchDedup())
    model.last_primitive.n_prim      # [512] atoms per structure after the reduction
    atoms[0].info["primitive"]       # the structure's record as a dict

    natoms_p, a_p, x_p, lat_p, report = primitive_states(natoms, a, x, lat, Primitive(symprec=0.05))
    symmetry_states(natoms_p, a_p, x_p, lat_p)          # the crystal system of the primitive cells

Per crystal: the pure translations that carry the atoms onto themselves within `symprec` (the search of
chemeleon_amd.symmetry with W = I), the Hermite normal form H of the integer lattice they span, the cell
Lp = H Lr / m and one atom per orbit, the one of the lowest index with the coordinates it has. A set of
translations that is no group halves the tolerance, at most four times. A crystal without such translations, or
with a flag, comes back as it is in its Niggli-reduced basis.

This is not a port of spglib's find_primitive, and how far the two agree on real samples has not been measured.
There is no averaging over an orbit, no standardised (conventional) cell and no space-group number (DESIGN.md §4,
"Primitive cells").
"""

from typing import Optional, Sequence

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd import cell as _cell
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state

AMBIGUOUS, NO_LATTICE, THIN = 1, 4, 8
FLAG_NAMES = {AMBIGUOUS: "ambiguous", NO_LATTICE: "no_lattice", THIN: "thin"}
RECORD_BYTES = 64
MAX_ATOMS = 256
MAX_SYMPREC, MAX_ANGLE_TOLERANCE = _cell.MAX_SYMPREC, _cell.MAX_ANGLE_TOLERANCE


class Primitive:
    """How a finished structure's primitive cell is found: `symprec` (A, at most 1) is the distance within which
    a translated atom must land on one of its kind, and with `angle_tolerance` (degrees, at most 30) the tolerance
    of the lattice search in front of it (the defaults are the reference's). Validated here, on the host
    (ValueError)."""

    def __init__(self, symprec: float = 0.1, angle_tolerance: float = 10.0):
        for name, v, top in (("symprec", symprec, MAX_SYMPREC), ("angle_tolerance", angle_tolerance, MAX_ANGLE_TOLERANCE)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not 0 < float(np.float32(v)) <= top:
                raise ValueError(f"{name} must be in (0, {top:g}], got {v!r}")
        self.symprec, self.angle_tolerance = float(symprec), float(angle_tolerance)

    def __repr__(self):
        return f"Primitive(symprec={self.symprec}, angle_tolerance={self.angle_tolerance})"


class PrimitiveReport:
    """The records of one batch as numpy arrays: n_prim [B] (atoms written per crystal), n_trans [B] (m), n_pivot,
    halvings, flags [B], hnf [B,3,3] int64 (H, upper triangular; the identity where the crystal was passed
    through), tol [B], lattice_code [B] and lattice_system [B] (cell.SYSTEMS names, of the input cell), reduced [B]
    (bool: n_prim < n), valid [B] (flags == 0) and natoms [B] (the input's)."""

    def __init__(self, records: np.ndarray, natoms: Sequence[int]):
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        i = rec.view(np.int32)
        self.records = rec
        self.natoms = np.asarray(natoms, dtype=np.int32)
        self.n_prim = i[:, 0].copy()
        self.n_trans = i[:, 1].copy()
        self.n_pivot = i[:, 2].copy()
        self.halvings = i[:, 3].copy()
        self.flags = i[:, 4].copy()
        self.hnf = np.zeros((len(rec), 3, 3), dtype=np.int64)
        for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            self.hnf[:, r, c] = i[:, 5 + k]
        self.tol = rec.view(np.float32)[:, 11].copy()
        self.lattice_code = i[:, 12].copy()
        self.lattice_system = np.array([_cell.SYSTEMS[c] if 0 <= c < len(_cell.SYSTEMS) else ""
                                        for c in self.lattice_code])
        self.reduced = self.n_prim < self.natoms
        self.valid = self.flags == 0

    def __len__(self):
        return len(self.flags)

    def record(self, g: int) -> dict:
        """Crystal g's record as a dict of Python numbers (what sample() stores in atoms.info["primitive"])."""
        fl = int(self.flags[g])
        return {"n_prim": int(self.n_prim[g]), "natoms": int(self.natoms[g]), "n_trans": int(self.n_trans[g]),
                "n_pivot": int(self.n_pivot[g]), "halvings": int(self.halvings[g]), "flags": fl,
                "hnf": tuple(tuple(int(v) for v in row) for row in self.hnf[g]), "tol": float(self.tol[g]),
                "lattice_system": str(self.lattice_system[g]) or None, "reduced": bool(self.reduced[g]),
                "failed": [name for bit, name in FLAG_NAMES.items() if fl & bit], "valid": bool(self.valid[g])}


class PrimitivePlan(Plan):
    """Owns a chm_prim: the node offsets of one crystal list on one device."""

    _create, _destroy = "chm_prim_create", "chm_prim_destroy"

    def run(self, cell_records, atom_types, frac_coords, lattices, symprec: float, angle_tolerance: float, out,
            source, new_offsets, atom_types_out, frac_out, lattices_out):
        """Enqueues the three kernels on the current stream of the plan's device: `cell_records` is the output of
        a CellPlan.run on the same lattices and tolerances, `out` a uint8 device tensor of 64 bytes per crystal,
        `source` int32 [N], `new_offsets` int32 [B+1], the three *_out tensors shaped like the state and not the
        state itself. No host wait."""
        _lib.check(_lib.load().chm_prim_run(
            self.handle, _lib.ptr(cell_records), cell_records.numel(), _lib.ptr(atom_types), atom_types.numel(),
            _lib.ptr(frac_coords), frac_coords.numel(), _lib.ptr(lattices), lattices.numel(), float(symprec),
            float(angle_tolerance), _lib.ptr(out), out.numel(), _lib.ptr(source), source.numel(),
            _lib.ptr(new_offsets), new_offsets.numel(), _lib.ptr(atom_types_out), atom_types_out.numel(),
            _lib.ptr(frac_out), frac_out.numel(), _lib.ptr(lattices_out), lattices_out.numel(),
            _lib.stream_handle(self.device)), "chm_prim_run")
        return out


_plans = PlanCache(PrimitivePlan)


def primitive_plan(natoms: Sequence[int], device) -> PrimitivePlan:
    """The plan of this crystal list on this device, cached per (natoms, device) (the last 8)."""
    return _plans.get(device, natoms)


def primitive_states(natoms: Sequence[int], atom_types, frac_coords, lattices, primitive: Optional[Primitive] = None):
    """Reduces a state that lives on the device (atom_types [N] int64, frac_coords [N,3] and lattices [B,3,3] fp32,
    in node order of `natoms`; at most 256 atoms per crystal) to primitive cells and returns (natoms_p, a_p, x_p,
    lat_p, PrimitiveReport): the new crystal list and the state of N' = sum(natoms_p) atoms on the same device, the
    input untouched. The cell pass and the primitive pass are enqueued on one stream and only the 64-byte records
    cross to the host; the returned tensors are the first N' rows of the buffers the kernels packed. CPU tensors
    are refused: there is no host path."""
    if primitive is None:
        primitive = Primitive()
    if not isinstance(primitive, Primitive):
        raise ValueError("primitive must be a chemeleon_amd.Primitive")
    nat = check_natoms(natoms)
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices)
    cells, plan = _cell.cell_plan(nat, dev), primitive_plan(nat, dev)
    with torch.cuda.device(dev):
        cell_rec = torch.empty(B * _cell.RECORD_BYTES, dtype=torch.uint8, device=dev)
        out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
        source = torch.empty(N, dtype=torch.int32, device=dev)
        new_off = torch.empty(B + 1, dtype=torch.int32, device=dev)
        a_p, x_p, lat_p = torch.empty_like(atom_types), torch.empty_like(frac_coords), torch.empty_like(lattices)
        cells.run(lattices, None, primitive.symprec, primitive.angle_tolerance, cell_rec)
        plan.run(cell_rec, atom_types, frac_coords, lattices, primitive.symprec, primitive.angle_tolerance, out, source,
                 new_off, a_p, x_p, lat_p)
        host = out.cpu().numpy()  # (waits for the kernels; cell_rec, source and new_off stay alive until here)
    report = PrimitiveReport(host, nat)
    n_new = int(report.n_prim.sum())
    return [int(v) for v in report.n_prim], a_p[:n_new], x_p[:n_new], lat_p, report
