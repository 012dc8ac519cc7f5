"""Trajectory containers and structure output (reference
`chemeleon/modules/schema.py:14-88`).

`get_atoms` returns `ase.Atoms` when ase is importable, otherwise a minimal
`Atoms` with the same fields the reference callers use (numbers, cell, pbc,
scaled positions, chemical symbols / formula). In both cases the atoms of
each structure are sorted by chemical symbol (stable), as
`ase.build.tools.sort` does in the reference (schema.py:81).
"""

from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, List, Optional, Union

import numpy as np
import torch

CHEMICAL_SYMBOLS = (
    "X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se "
    "Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho "
    "Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm "
    "Md No Lr"
).split()

try:  # pragma: no cover - ase is not installed in this image
    from ase import Atoms as _AseAtoms
    from ase.build.tools import sort as _ase_sort
except Exception:  # noqa: BLE001
    _AseAtoms = None
    _ase_sort = None


class Atoms:
    """Minimal stand-in for ase.Atoms (used only when ase is unavailable)."""

    def __init__(self, numbers, cell, pbc=True, scaled_positions=None):
        self.numbers = np.asarray(numbers, dtype=np.int64)
        self.cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
        self.pbc = pbc
        self._scaled = (np.zeros((len(self.numbers), 3)) if scaled_positions is None
                        else np.asarray(scaled_positions, dtype=np.float64))

    def __len__(self):
        return len(self.numbers)

    def set_scaled_positions(self, p):
        self._scaled = np.asarray(p, dtype=np.float64)

    def get_scaled_positions(self, wrap=True):
        return self._scaled.copy()

    def get_positions(self):
        return self._scaled @ self.cell

    def get_atomic_numbers(self):
        return self.numbers.copy()

    def get_chemical_symbols(self):
        return [CHEMICAL_SYMBOLS[int(z)] for z in self.numbers]

    def get_chemical_formula(self):
        syms = self.get_chemical_symbols()
        return "".join(f"{s}{syms.count(s) if syms.count(s) > 1 else ''}" for s in sorted(set(syms)))

    def __getitem__(self, idx):
        return Atoms(self.numbers[idx], self.cell, self.pbc, self._scaled[idx])

    def __repr__(self):
        return f"Atoms(symbols='{self.get_chemical_formula()}', pbc={self.pbc})"


def sort_atoms(atoms):
    """ase.build.tools.sort: stable sort by chemical symbol."""
    if _ase_sort is not None and not isinstance(atoms, Atoms):
        return _ase_sort(atoms)
    tags = atoms.get_chemical_symbols()
    order = [i for _, i in sorted((tag, i) for i, tag in enumerate(tags))]
    return atoms[order]


def make_atoms(numbers, cell, scaled):
    if _AseAtoms is not None:
        at = _AseAtoms(numbers=numbers, cell=cell, pbc=True)
        at.set_scaled_positions(scaled)
        return at
    return Atoms(numbers, cell, True, scaled)


@dataclass
class TrajectoryStep:
    """schema.py:14-24"""
    num_atoms: torch.Tensor
    atom_types: torch.Tensor
    frac_coords: torch.Tensor
    lattices: torch.Tensor
    batch_idx: torch.Tensor
    atom_types_probs: Optional[torch.Tensor] = None


class TrajectoryContainer:
    """schema.py:26-88: time step -> TrajectoryStep."""

    def __init__(self, total_steps: int):
        self.total_steps = total_steps
        self.trajectory_continaer: Dict[int, Optional[TrajectoryStep]] = OrderedDict(
            (t, None) for t in range(total_steps))

    def __setitem__(self, t: int, step: TrajectoryStep) -> None:
        self.trajectory_continaer[t] = step

    def __getitem__(self, t: int) -> TrajectoryStep:
        if t == -1:
            t = self.total_steps
        return self.trajectory_continaer[t]

    def __len__(self):
        return len(self.trajectory_continaer)

    def __iter__(self):
        return iter(self.trajectory_continaer)

    def get_atoms(self, t: int = 0, idx: int = None):
        st = self[t]
        return step_to_atoms(st.atom_types, st.frac_coords, st.lattices, st.num_atoms, idx)

    def get_trajectory(self, idx: int = None):
        return [self.get_atoms(t, idx) for t in range(self.total_steps + 1)]


def step_to_atoms(atom_types, frac_coords, lattices, num_atoms, idx: int = None) -> Union[List, object]:
    """schema.py:57-83: split per crystal, clamp classes > 103 to 0, build
    Atoms(numbers, cell, pbc) with scaled positions, sort by symbol."""
    a = atom_types.detach().cpu()
    a = torch.where(a <= 103, a, 0).numpy()
    x = frac_coords.detach().cpu().numpy()
    lat = lattices.detach().cpu().numpy()
    nat = [int(n) for n in (num_atoms.tolist() if torch.is_tensor(num_atoms) else num_atoms)]
    out, off = [], 0
    for g, n in enumerate(nat):
        out.append(sort_atoms(make_atoms(a[off:off + n], lat[g], x[off:off + n])))
        off += n
    return out if idx is None else out[idx]


# ---------------------------------------------------------------------------------------------
# Streaming output: the state snapshot made on the device (chm_snapshot_*, include/chemeleon_hip.h)
# and the structures sliced out of it.
# ---------------------------------------------------------------------------------------------
def symbol_rank_table() -> np.ndarray:
    """rank[z] = position of CHEMICAL_SYMBOLS[z] among the sorted symbols (uint8 [104]): the sort key
    of the device snapshot, so that sorting by it is sorting by symbol as `sort_atoms` does."""
    order = sorted(range(len(CHEMICAL_SYMBOLS)), key=lambda z: CHEMICAL_SYMBOLS[z])
    rank = np.empty(len(CHEMICAL_SYMBOLS), dtype=np.uint8)
    rank[order] = np.arange(len(CHEMICAL_SYMBOLS), dtype=np.uint8)
    return rank


def slot_layout(natoms) -> Dict[str, int]:
    """Byte offsets of one packed snapshot slot (include/chemeleon_hip.h): lattices f32 [B*9], frac f32
    [N*3] (sorted), perm i32 [N], numbers u8 [N] (sorted); `bytes` = the slot size, a multiple of 16."""
    B, N = len(natoms), int(sum(natoms))
    lay = {"lattices": 0, "frac": 36 * B, "perm": 36 * B + 12 * N, "numbers": 36 * B + 16 * N}
    lay["bytes"] = (36 * B + 17 * N + 15) // 16 * 16
    return lay


def slot_to_atoms(slot, natoms) -> List:
    """The structures of one packed host slot (a uint8 buffer of `slot_layout(natoms)["bytes"]` bytes: a
    numpy array, a CPU torch tensor or anything with the buffer protocol): what `step_to_atoms` returns for
    the state the slot was made from. The atoms are already clamped and sorted, so each structure is a
    slice; every array is copied out of the slot (astype), which its owner reuses for a later step."""
    if torch.is_tensor(slot):
        slot = slot.numpy()
    buf = np.frombuffer(slot, dtype=np.uint8)
    nat = [int(n) for n in (natoms.tolist() if torch.is_tensor(natoms) else natoms)]
    B, N = len(nat), sum(nat)
    lay = slot_layout(nat)
    if buf.size != lay["bytes"]:
        raise ValueError(f"slot of {buf.size} bytes, these crystals need {lay['bytes']}")
    lat = buf[:lay["frac"]].view(np.float32).reshape(B, 3, 3)
    x = buf[lay["frac"]:lay["perm"]].view(np.float32).reshape(N, 3)
    num = buf[lay["numbers"]:lay["numbers"] + N]
    out, off = [], 0
    for g, n in enumerate(nat):
        out.append(make_atoms(num[off:off + n].astype(np.int64), lat[g].astype(np.float64),
                              x[off:off + n].astype(np.float64)))
        off += n
    return out


class StateStreamer:
    """Hands sampler states to the host as structure lists without stalling the sampler.

    A ring of `slots` (>= 2) device slots with matching pinned host slots, a copy stream and per-slot
    events. `push(a, x, lat)` enqueues the snapshot kernel on the CURRENT stream (so, called between two
    replays of the reverse step, it reads the state the first one produced), then the slot's copy to
    pinned memory on the copy stream behind an event; before a device slot is written again the compute
    stream waits, on the device, for the copy that last read it. `pop(ticket)` blocks the host on that
    slot's copy event only and returns `slot_to_atoms` of it (copied out: the slot is reused). A slot
    pushed again before it was popped is an error."""

    def __init__(self, natoms, device, slots: int = 2):
        from chemeleon_amd import _lib
        import ctypes
        if slots < 2:
            raise ValueError("StateStreamer needs a ring of at least 2 slots")
        self._lib = _lib
        self.natoms = [int(n) for n in natoms]
        self.device = torch.device(device)
        nat = (ctypes.c_int32 * len(self.natoms))(*self.natoms)
        rank = symbol_rank_table()
        plan = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().chm_snapshot_create(
                nat, len(self.natoms), rank.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(rank),
                ctypes.byref(plan)), "chm_snapshot_create")
        self._plan = plan
        self.slot_bytes = int(_lib.load().chm_snapshot_slot_bytes(plan))
        assert self.slot_bytes == slot_layout(self.natoms)["bytes"]
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._dev = [torch.empty(self.slot_bytes, dtype=torch.uint8, device=self.device) for _ in range(slots)]
        for d in self._dev:  # (read on the copy stream: the allocator must not hand the block on before that)
            d.record_stream(self.copy_stream)
        self._pin = [torch.empty(self.slot_bytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self._snapped = [torch.cuda.Event() for _ in range(slots)]
        self._copied = [torch.cuda.Event() for _ in range(slots)]
        self._busy = [False] * slots      # pushed, not yet popped
        self._used = [False] * slots      # _copied[k] has been recorded
        self.uses = [0] * slots           # pushes per slot
        self._head = 0

    def push(self, atom_types, frac_coords, lattices) -> int:
        """Snapshot of this state into the next slot; returns the ticket for `pop`. No host wait."""
        L = self._lib
        k = self._head % len(self._dev)
        if self._busy[k]:
            raise RuntimeError("StateStreamer: every slot of the ring holds a state that was not popped")
        L.require_device(atom_types, frac_coords, lattices)
        cur = torch.cuda.current_stream(self.device)
        if self._used[k]:
            cur.wait_event(self._copied[k])
        L.check(L.load().chm_snapshot_run(
            self._plan, L.ptr(atom_types), atom_types.numel(), L.ptr(frac_coords), frac_coords.numel(),
            L.ptr(lattices), lattices.numel(), L.ptr(self._dev[k]), self.slot_bytes,
            L.c_void_p(cur.cuda_stream)), "chm_snapshot_run")
        self._snapped[k].record(cur)
        self.copy_stream.wait_event(self._snapped[k])
        with torch.cuda.stream(self.copy_stream):
            self._pin[k].copy_(self._dev[k], non_blocking=True)
        self._copied[k].record(self.copy_stream)
        self._busy[k], self._used[k] = True, True
        self.uses[k] += 1
        self._head += 1
        return k

    def pop(self, ticket: int) -> List:
        """The structures of the state pushed as `ticket`; blocks the host until that slot's copy is done."""
        if not self._busy[ticket]:
            raise RuntimeError("StateStreamer: this slot holds no pushed state")
        self._copied[ticket].synchronize()
        out = slot_to_atoms(self._pin[ticket].numpy(), self.natoms)
        self._busy[ticket] = False
        return out

    def close(self):
        if self._plan is not None:
            self.copy_stream.synchronize()
            self._lib.load().chm_snapshot_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass


# ---------------------------------------------------------------------------------------------
# CIF output (the reference's scripts convert the sampled ase.Atoms with pymatgen's
# AseAtomsAdaptor and write `gen_{i}.cif`, chemeleon/scripts/sample_prompt.py:38-42; neither
# pymatgen nor ase is needed here): P1 cell + fractional coordinates + symbols.
# ---------------------------------------------------------------------------------------------
def cell_parameters(cell) -> tuple:
    """(a, b, c, alpha, beta, gamma) in Angstrom / degrees of a row-vector cell [3, 3]."""
    v = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    lens = np.linalg.norm(v, axis=1)

    def ang(i, j):
        d = lens[i] * lens[j]
        return 90.0 if d == 0 else float(np.degrees(np.arccos(np.clip(np.dot(v[i], v[j]) / d, -1.0, 1.0))))

    return float(lens[0]), float(lens[1]), float(lens[2]), ang(1, 2), ang(0, 2), ang(0, 1)


def _formula_counts(symbols):
    counts: Dict[str, int] = OrderedDict()
    for s in symbols:
        counts[s] = counts.get(s, 0) + 1
    return counts


def atoms_to_cif(atoms, name: Optional[str] = None) -> str:
    """One structure (ase.Atoms or this module's Atoms) as a P1 CIF document."""
    symbols = list(atoms.get_chemical_symbols())
    frac = np.asarray(atoms.get_scaled_positions(), dtype=np.float64).reshape(-1, 3)
    a, b, c, al, be, ga = cell_parameters(np.asarray(atoms.cell))
    vol = float(abs(np.linalg.det(np.asarray(atoms.cell, dtype=np.float64).reshape(3, 3))))
    counts = _formula_counts(sorted(symbols))
    formula_sum = " ".join(f"{s}{n}" for s, n in counts.items())
    name = name or "".join(f"{s}{n}" for s, n in counts.items())
    lines = [
        f"data_{name}",
        "_symmetry_space_group_name_H-M   'P 1'",
        f"_cell_length_a   {a:.8f}",
        f"_cell_length_b   {b:.8f}",
        f"_cell_length_c   {c:.8f}",
        f"_cell_angle_alpha   {al:.8f}",
        f"_cell_angle_beta   {be:.8f}",
        f"_cell_angle_gamma   {ga:.8f}",
        "_symmetry_Int_Tables_number   1",
        f"_chemical_formula_structural   {name}",
        f"_chemical_formula_sum   '{formula_sum}'",
        f"_cell_volume   {vol:.8f}",
        "_cell_formula_units_Z   1",
        "loop_",
        " _symmetry_equiv_pos_site_id",
        " _symmetry_equiv_pos_as_xyz",
        "  1  'x, y, z'",
        "loop_",
        " _atom_site_type_symbol",
        " _atom_site_label",
        " _atom_site_symmetry_multiplicity",
        " _atom_site_fract_x",
        " _atom_site_fract_y",
        " _atom_site_fract_z",
        " _atom_site_occupancy",
    ]
    seen: Dict[str, int] = {}
    for s, (x, y, z) in zip(symbols, frac):
        k = seen.get(s, 0)
        seen[s] = k + 1
        lines.append(f"  {s}  {s}{k}  1  {x:.8f}  {y:.8f}  {z:.8f}  1")
    return "\n".join(lines) + "\n"


def write_cif(atoms, path) -> str:
    """Writes one structure to `path` (a .cif file); returns the path."""
    path = str(path)
    with open(path, "w") as f:
        f.write(atoms_to_cif(atoms))
    return path


def save_structures(atoms_list, save_dir, prefix: str = "gen_") -> List[str]:
    """The reference's output step (sample_prompt.py:38-42): `save_dir/gen_{i}.cif` per structure."""
    import os
    os.makedirs(str(save_dir), exist_ok=True)
    return [write_cif(at, os.path.join(str(save_dir), f"{prefix}{i}.cif")) for i, at in enumerate(atoms_list)]
