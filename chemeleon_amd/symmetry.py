"""Crystal system with the atoms of sampled structures on the device.

The reference's scripts/evaluate.py asks pymatgen / spglib on the host which crystal system a generated structure
has (`test_crystal_system_matching`: SpacegroupAnalyzer(st, symprec=0.1, angle_tolerance=10).get_crystal_system()),
and its models take the crystal system as a text target. Here the final state is classified where it already is
(the kernel is csrc/symm.hip; the definition is in include/chemeleon_hip.h at chm_symm_*):

    atoms = model.sample("cubic", 8, 512, noise="philox", symmetry=Symmetry(require="cubic"))
    model.last_symmetry.system       # [512] names: what every sample came out as; `atoms` holds the cubic ones
    atoms[0].info["symmetry"]        # the structure's record as a dict

    report = symmetry_states(natoms, a, x, lat, Symmetry(symprec=0.05), operations=True)   # device -> numpy

Per crystal: the lattice operations W that the cell search (chemeleon_amd.cell) accepted, and for each of them the
translations that carry the atoms onto themselves within `symprec`, tried from the atoms of the rarest species.
The rotation parts of the accepted pairs name the rotation group of the Laue class and that names the system; a
set that is no group halves the tolerance, at most four times. Code 4 is "trigonal" here (pymatgen's name) and
"rhombohedral" in cell.SYSTEMS: alpha-quartz is trigonal on a hexagonal lattice.

This is not a port of spglib, and how far the two agree on real samples has not been measured. There is no
reduction to a primitive cell: with n_trans > 1 the answer describes the cell as given, so a supercell whose
lattice has lower symmetry than the primitive lattice (a 2x1x1 cell of CsCl) reports the lower system; the way
round it is chemeleon_amd.primitive (primitive_states, or sample(primitive=...)), which runs first. The
space-group number and the point group's name are not built ("Crystal system with the atoms").
"""

from typing import Optional, Sequence, Union

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd import cell as _cell
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state

CRYSTAL_SYSTEMS = ("triclinic", "monoclinic", "orthorhombic", "tetragonal", "trigonal", "hexagonal", "cubic")
AMBIGUOUS, MISMATCH, NO_LATTICE, THIN = 1, 2, 4, 8
FLAG_NAMES = {AMBIGUOUS: "ambiguous", MISMATCH: "mismatch", NO_LATTICE: "no_lattice", THIN: "thin"}
RECORD_BYTES = 64
MAX_OPS = 48
MAX_ATOMS = 256
MAX_SYMPREC, MAX_ANGLE_TOLERANCE = _cell.MAX_SYMPREC, _cell.MAX_ANGLE_TOLERANCE


def crystal_system_code(name) -> int:
    """"cubic" -> 6; ValueError for anything that is not one of CRYSTAL_SYSTEMS."""
    if not isinstance(name, str) or name not in CRYSTAL_SYSTEMS:
        raise ValueError(f"unknown crystal system {name!r}: expected one of {', '.join(CRYSTAL_SYSTEMS)}")
    return CRYSTAL_SYSTEMS.index(name)


def candidate_matrix(index) -> np.ndarray:
    """The integer matrix W [3,3] of a candidate index of the search (its base-3 digits, least significant first,
    are the row-major entries + 1)."""
    index = int(index)
    if not 0 <= index < 3 ** 9:
        raise ValueError(f"candidate index {index} outside [0, 19683)")
    return np.array([(index // 3 ** q) % 3 - 1 for q in range(9)], dtype=np.int64).reshape(3, 3)


class Symmetry:
    """How a finished structure's crystal system is found: `symprec` (A, at most 1) is the distance within which
    an atom must land on one of its kind, and with `angle_tolerance` (degrees, at most 30) the tolerance of the
    lattice search (the defaults are the reference's). `require` names the crystal system a structure must have
    (one name for every crystal, or a list with one name per crystal; a structure without a system never meets
    it). Everything is validated here, on the host (ValueError)."""

    def __init__(self, symprec: float = 0.1, angle_tolerance: float = 10.0,
                 require: Optional[Union[str, Sequence[str]]] = None):
        for name, v, top in (("symprec", symprec, MAX_SYMPREC), ("angle_tolerance", angle_tolerance, MAX_ANGLE_TOLERANCE)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"{name} must be a number, got {v!r}")
            if not 0 < float(np.float32(v)) <= top:
                raise ValueError(f"{name} must be in (0, {top:g}], got {v!r}")
        self.symprec, self.angle_tolerance = float(symprec), float(angle_tolerance)
        self.require = require
        if require is None:
            self.codes = None
        elif isinstance(require, str):
            self.codes = np.array([crystal_system_code(require)], dtype=np.int32)
        else:
            try:
                names = list(require)
            except TypeError:
                raise ValueError(f"require must be a crystal system's name or a list of them, got {require!r}") from None
            if not names:
                raise ValueError("require: an empty list of crystal systems")
            self.codes = np.array([crystal_system_code(n) for n in names], dtype=np.int32)
        self._per_crystal = require is not None and not isinstance(require, str)

    def codes_for(self, num_graphs: int) -> Optional[np.ndarray]:
        """The int32 required codes of a batch of num_graphs crystals ([1], [num_graphs] or None); ValueError if
        a per-crystal list has another length."""
        if self._per_crystal and len(self.codes) != num_graphs:
            raise ValueError(f"require lists {len(self.codes)} crystal systems, the batch has {num_graphs} crystals")
        return self.codes

    def __repr__(self):
        return f"Symmetry(symprec={self.symprec}, angle_tolerance={self.angle_tolerance}, require={self.require!r})"


class SymmetryReport:
    """The records of one batch as numpy arrays: system [B] (names; "" where none), code [B] (-1 where none),
    n_sym, n_trans, n_pg, n_proper [B], orders [B,4] (n2, n3, n4, n6 of the proper parts), inversion [B] (bool),
    halvings, flags, n_pivot [B], lattice_code [B] and lattice_system [B] (cell.SYSTEMS names), tol [B], mismatch
    [B] (a required system was not met) and valid [B] (flags == 0 and a system was found). `operations` is None,
    or, if they were asked for, a list with one (indices [n_pg], W [n_pg,3,3] int64, t [n_pg,3] float32) per
    crystal: x -> x W + t in the Niggli-reduced basis."""

    def __init__(self, records: np.ndarray, operations: Optional[np.ndarray] = None):
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        i = rec.view(np.int32)
        self.records = rec
        self.code = i[:, 0].copy()
        self.n_sym = i[:, 1].copy()
        self.n_trans = i[:, 2].copy()
        self.n_pg = i[:, 3].copy()
        self.n_proper = i[:, 4].copy()
        self.orders = i[:, 5:9].copy()
        self.inversion = i[:, 9] != 0
        self.halvings = i[:, 10].copy()
        self.flags = i[:, 11].copy()
        self.n_pivot = i[:, 12].copy()
        self.lattice_code = i[:, 13].copy()
        self.tol = rec.view(np.float32)[:, 14].copy()
        self.system = np.array([CRYSTAL_SYSTEMS[c] if 0 <= c < len(CRYSTAL_SYSTEMS) else "" for c in self.code])
        self.lattice_system = np.array([_cell.SYSTEMS[c] if 0 <= c < len(_cell.SYSTEMS) else ""
                                        for c in self.lattice_code])
        self.mismatch = (self.flags & MISMATCH) != 0
        self.valid = (self.flags == 0) & (self.code >= 0)
        self.operations = None
        if operations is not None:
            raw = np.ascontiguousarray(operations, dtype=np.uint8).reshape(len(rec), MAX_OPS, 16)
            self.operation_slots = raw
            idx = raw.view(np.int32)[:, :, 0]
            tr = raw.view(np.float32)[:, :, 1:4]
            self.operations = []
            for g in range(len(rec)):
                used = idx[g] >= 0
                W = np.stack([candidate_matrix(v) for v in idx[g][used]]) if used.any() else np.zeros((0, 3, 3), np.int64)
                self.operations.append((idx[g][used].copy(), W, tr[g][used].copy()))

    def __len__(self):
        return len(self.flags)

    def record(self, g: int) -> dict:
        """Crystal g's record as a dict of Python numbers (what sample() stores in atoms.info["symmetry"])."""
        fl = int(self.flags[g])
        return {"system": str(self.system[g]) or None, "code": int(self.code[g]), "n_sym": int(self.n_sym[g]),
                "n_trans": int(self.n_trans[g]), "n_pg": int(self.n_pg[g]), "n_proper": int(self.n_proper[g]),
                "orders": tuple(int(v) for v in self.orders[g]), "inversion": bool(self.inversion[g]),
                "halvings": int(self.halvings[g]), "flags": fl, "n_pivot": int(self.n_pivot[g]),
                "lattice_system": str(self.lattice_system[g]) or None, "tol": float(self.tol[g]),
                "failed": [name for bit, name in FLAG_NAMES.items() if fl & bit], "valid": bool(self.valid[g])}


class SymmetryPlan(Plan):
    """Owns a chm_symm: the node offsets of one crystal list on one device."""

    _create, _destroy = "chm_symm_create", "chm_symm_destroy"

    def run(self, cell_records, atom_types, frac_coords, lattices, require, symprec: float, angle_tolerance: float,
            out, ops=None):
        """Enqueues the search on the current stream of the plan's device: `cell_records` is the output of a
        CellPlan.run on the same lattices and tolerances, `out` a uint8 device tensor of 64 bytes per crystal,
        `ops` None or one of 768 bytes per crystal, `require` an int32 device tensor or None. No host wait."""
        _lib.check(_lib.load().chm_symm_run(
            self.handle, _lib.ptr(cell_records), cell_records.numel(), _lib.ptr(atom_types), atom_types.numel(),
            _lib.ptr(frac_coords), frac_coords.numel(), _lib.ptr(lattices), lattices.numel(), _lib.ptr(require),
            0 if require is None else require.numel(), float(symprec), float(angle_tolerance), _lib.ptr(out),
            out.numel(), _lib.ptr(ops), 0 if ops is None else ops.numel(), _lib.stream_handle(self.device)),
            "chm_symm_run")
        return out


_plans = PlanCache(SymmetryPlan)


def symmetry_plan(natoms: Sequence[int], device) -> SymmetryPlan:
    """The plan of this crystal list on this device, cached per (natoms, device) (the last 8)."""
    return _plans.get(device, natoms)


def symmetry_states(natoms: Sequence[int], atom_types, frac_coords, lattices, symmetry: Optional[Symmetry] = None,
                    operations: bool = False) -> SymmetryReport:
    """Finds the crystal systems of a state that lives on the device (atom_types [N] int64, frac_coords [N,3] and
    lattices [B,3,3] fp32, in node order of `natoms`; at most 256 atoms per crystal) and returns its
    SymmetryReport: the cell pass and the symmetry pass are enqueued on one stream and only the 64-byte records
    (and the operations, if asked for) cross to the host. CPU tensors are refused: there is no host path."""
    if symmetry is None:
        symmetry = Symmetry()
    if not isinstance(symmetry, Symmetry):
        raise ValueError("symmetry must be a chemeleon_amd.Symmetry")
    nat = check_natoms(natoms)
    codes = symmetry.codes_for(len(nat))
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices)
    cells, plan = _cell.cell_plan(nat, dev), symmetry_plan(nat, dev)
    with torch.cuda.device(dev):
        rq = None if codes is None else torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
        cell_rec = torch.empty(B * _cell.RECORD_BYTES, dtype=torch.uint8, device=dev)
        out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
        ops = torch.empty(B * MAX_OPS * 16, dtype=torch.uint8, device=dev) if operations else None
        cells.run(lattices, None, symmetry.symprec, symmetry.angle_tolerance, cell_rec)
        plan.run(cell_rec, atom_types, frac_coords, lattices, rq, symmetry.symprec, symmetry.angle_tolerance, out, ops)
        host = out.cpu().numpy()  # (waits for the kernels; rq, cell_rec and out stay alive until here)
        host_ops = ops.cpu().numpy() if operations else None
    return SymmetryReport(host, host_ops)

