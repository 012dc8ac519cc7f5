"""Screening of sampled structures on the device: cell, shortest distance, formula.

The reference's sampling scripts screen every generated structure with pymatgen before anything else looks at
it (`test_valid` in scripts/evaluate.py: longest cell edge <= 60 A, shortest interatomic distance under periodic
boundaries >= 0.5 A; scripts/sample_target_composition.py: the reduced formula is the one asked for). Here the
final state is screened where it already is (the kernel is csrc/screen.hip, the record and its semantics are in
include/chemeleon_hip.h at chm_screen_record):

    atoms = model.sample("TiO2", 12, 64, noise="philox", screen=Screen(composition="TiO2"))
    model.last_screen.valid          # [64] bool: which samples passed; `atoms` holds only those
    atoms[0].info["screen"]          # the passing structure's record as a dict

    report = screen_states(natoms, a, x, lat, Screen(min_distance=0.7))   # device tensors -> numpy arrays

One deliberate difference from the reference's filter: its `np.min(dist_mat[dist_mat > 0])` ignores exactly
coincident atoms; here they give dmin = 0 and fail the screen.
"""

import math
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from chemeleon_amd import _lib
from chemeleon_amd._plans import Plan, PlanCache, check_natoms, check_state
from chemeleon_amd.constraints import MAX_ATOMS, parse_formula

TOO_LONG, TOO_CLOSE, COMPOSITION, DEGENERATE, NONFINITE = 1, 2, 4, 8, 16
RECORD_BYTES = 64
FLAG_NAMES = {TOO_LONG: "too_long", TOO_CLOSE: "too_close", COMPOSITION: "composition", DEGENERATE: "degenerate",
              NONFINITE: "nonfinite"}


def reduced_counts(formula: str) -> np.ndarray:
    """"Ti2O4" -> int32 [104] with 1 at Ti and 2 at O: the element counts divided by their gcd."""
    counts = parse_formula(formula)
    g = 0
    for c in counts.values():
        g = math.gcd(g, c)
    out = np.zeros(MAX_ATOMS, dtype=np.int32)
    for z, c in counts.items():
        out[z] = c // g
    return out


class Screen:
    """The criteria a finished structure must meet: longest cell edge <= max_length (A), shortest periodic
    interatomic distance >= min_distance (A) and, with `composition` (one formula string for every crystal, or
    a list with one formula per crystal), the reduced formula equal to that formula's. Everything is validated
    here, on the host (ValueError)."""

    def __init__(self, max_length: float = 60.0, min_distance: float = 0.5,
                 composition: Optional[Union[str, Sequence[str]]] = None):
        self.max_length, self.min_distance = float(max_length), float(min_distance)
        if not (self.max_length > 0 and math.isfinite(self.max_length)):
            raise ValueError(f"max_length must be a positive length, got {max_length!r}")
        if not (self.min_distance > 0 and math.isfinite(self.min_distance)):
            raise ValueError(f"min_distance must be a positive length, got {min_distance!r}")
        self.composition = composition
        if composition is None:
            self.target = None
        elif isinstance(composition, str):
            self.target = reduced_counts(composition)
        else:
            rows = [reduced_counts(f) for f in composition]
            if not rows:
                raise ValueError("composition: an empty list of formulas")
            self.target = np.stack(rows)

    def target_for(self, num_graphs: int) -> Optional[np.ndarray]:
        """The int32 target of a batch of num_graphs crystals ([104], [num_graphs,104] or None); ValueError
        if a per-crystal list has another length."""
        if self.target is not None and self.target.ndim == 2 and self.target.shape[0] != num_graphs:
            raise ValueError(f"composition lists {self.target.shape[0]} formulas, the batch has {num_graphs} crystals")
        return self.target

    def __repr__(self):
        return (f"Screen(max_length={self.max_length}, min_distance={self.min_distance}, "
                f"composition={self.composition!r})")


class ScreenReport:
    """The records of one screened batch as numpy arrays: lengths [B,3], angles [B,3] (alpha, beta, gamma in
    degrees), volume [B], dmin [B], pair [B,2] (a pair that attains dmin; -1, -1 for one atom), formula_units
    [B], flags [B] and valid [B] (flags == 0)."""

    def __init__(self, records: np.ndarray):
        rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, RECORD_BYTES)
        f = rec.view(np.float32)
        i = rec.view(np.int32)
        self.records = rec
        self.lengths = f[:, 0:3].copy()
        self.angles = f[:, 3:6].copy()
        self.volume = f[:, 6].copy()
        self.dmin = f[:, 7].copy()
        self.pair = i[:, 8:10].copy()
        self.formula_units = i[:, 10].copy()
        self.flags = i[:, 11].copy()
        self.valid = self.flags == 0

    def __len__(self):
        return len(self.flags)

    def record(self, g: int) -> dict:
        """Crystal g's record as a dict of Python numbers (what sample() stores in atoms.info["screen"])."""
        fl = int(self.flags[g])
        return {"lengths": tuple(float(v) for v in self.lengths[g]), "angles": tuple(float(v) for v in self.angles[g]),
                "volume": float(self.volume[g]), "dmin": float(self.dmin[g]),
                "pair": (int(self.pair[g, 0]), int(self.pair[g, 1])), "formula_units": int(self.formula_units[g]),
                "flags": fl, "failed": [name for bit, name in FLAG_NAMES.items() if fl & bit], "valid": fl == 0}


class ScreenPlan(Plan):
    """Owns a chm_screen: the node offsets of one crystal list on one device."""

    _create, _destroy = "chm_screen_create", "chm_screen_destroy"

    def run(self, atom_types, frac_coords, lattices, target, max_length: float, min_distance: float, out):
        """Enqueues the screen on the current stream of the plan's device; `out` is a uint8 device tensor of 64
        bytes per crystal, `target` an int32 device tensor or None. No host wait."""
        _lib.check(_lib.load().chm_screen_run(
            self.handle, _lib.ptr(atom_types), atom_types.numel(), _lib.ptr(frac_coords), frac_coords.numel(),
            _lib.ptr(lattices), lattices.numel(), _lib.ptr(target), 0 if target is None else target.numel(),
            float(max_length), float(min_distance), _lib.ptr(out), out.numel(), _lib.stream_handle(self.device)),
            "chm_screen_run")
        return out


_plans = PlanCache(ScreenPlan)


def screen_plan(natoms: Sequence[int], device) -> ScreenPlan:
    """The plan of this crystal list on this device, cached per (natoms, device) (the last 8)."""
    return _plans.get(device, natoms)


def screen_states(natoms: Sequence[int], atom_types, frac_coords, lattices, screen: Optional[Screen] = None
                  ) -> ScreenReport:
    """Screens a state that lives on the device (atom_types [N] int64, frac_coords [N,3] and lattices [B,3,3]
    fp32, in node order of `natoms`) and returns its ScreenReport; only the 64-byte records cross to the host.
    CPU tensors are refused: there is no host path."""
    screen = Screen() if screen is None else screen
    nat = check_natoms(natoms)
    target = screen.target_for(len(nat))
    N, B, dev = check_state(nat, atom_types, frac_coords, lattices)
    plan = screen_plan(nat, dev)
    with torch.cuda.device(dev):
        tg = None if target is None else torch.from_numpy(np.ascontiguousarray(target)).to(dev)
        out = torch.empty(B * RECORD_BYTES, dtype=torch.uint8, device=dev)
        plan.run(atom_types, frac_coords, lattices, tg, screen.max_length, screen.min_distance, out)
        host = out.cpu().numpy()  # (waits for the screen; tg and out stay alive until here)
    return ScreenReport(host)


def selected_atoms(natoms: Sequence[int], atom_types, frac_coords, lattices, keep: Sequence[int]):
    """The crystals `keep` (indices into natoms, in order) of a device state as structures: only their rows are
    copied and converted (schema.step_to_atoms); each gets an `info` dict if it has none."""
    from chemeleon_amd.modules.schema import step_to_atoms
    nat = [int(n) for n in natoms]
    offs = np.concatenate([[0], np.cumsum(nat)])
    rows = torch.cat([torch.arange(int(offs[g]), int(offs[g + 1])) for g in keep]).to(atom_types.device)
    graphs = torch.tensor(list(keep), device=lattices.device)
    atoms = step_to_atoms(atom_types.index_select(0, rows), frac_coords.index_select(0, rows),
                          lattices.index_select(0, graphs), [nat[g] for g in keep])
    for at in atoms:
        if getattr(at, "info", None) is None:
            at.info = {}
    return atoms


def screened_atoms(natoms: Sequence[int], atom_types, frac_coords, lattices, screen: Screen):
    """(passing structures, report): screens the state on the device, then copies and converts only the crystals
    that pass, each with atoms.info["screen"] = its record."""
    from chemeleon_amd.finish import finish_atoms
    atoms, reports = finish_atoms(natoms, atom_types, frac_coords, lattices, screen=Screen() if screen is None else screen)
    return atoms, reports["screen"]
