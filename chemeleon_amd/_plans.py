"""What the finishing legs (screening, cell, symmetry, dedup, match, match_group) share on the Python side: the
owner of a chm_* plan handle, the cache of the last plans per crystal list and device, and the validation of a
device state against its crystal list. A leg's module is its settings class, its report and the order of its
launches.

The lifetime rule: whoever runs a plan holds the plan object, so a plan that the cache evicts meanwhile is
destroyed only after its last user lets go of it.
"""

import ctypes
import threading
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np
import torch

from chemeleon_amd import _lib


def hip_device(device) -> torch.device:
    """`device` as a HIP device with an index (the current device where it has none); RuntimeError for any other."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("chemeleon_amd runs on a HIP device only: got " + str(dev))
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def int32_array(values: Sequence[int]):
    return (ctypes.c_int32 * len(values))(*values)


class Plan:
    """Owns one chm_* plan handle of a crystal list on one device. A subclass names its entry points in `_create`
    / `_destroy`; one whose chm_*_create takes more than (natoms, count, out) has its own __init__ around _make."""

    _create = _destroy = None
    handle = None

    def __init__(self, natoms: Sequence[int], device):
        self.natoms = tuple(int(n) for n in natoms)
        self.device = torch.device(device)
        self._make(int32_array(self.natoms), len(self.natoms))

    def _make(self, *args):
        h = _lib.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(_lib.load(), self._create)(*args, ctypes.byref(h)), self._create)
        self.handle = h

    def __del__(self):
        try:
            if self.handle:
                getattr(_lib.load(), self._destroy)(self.handle)
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass


class PlanCache:
    """The last 8 plans of one leg, keyed by its crystal lists and the device index; the oldest goes first.
    `factory(*lists, device)` builds a plan."""

    def __init__(self, factory):
        self._factory = factory
        self._plans = OrderedDict()
        self._lock = threading.Lock()

    def __len__(self):
        return len(self._plans)

    def get(self, device, *lists):
        dev = hip_device(device)
        key = tuple(tuple(map(int, values)) for values in lists) + (dev.index,)
        with self._lock:
            p = self._plans.get(key)
            if p is None:
                if len(self._plans) >= 8:
                    self._plans.popitem(last=False)
                p = self._plans[key] = self._factory(*key[:-1], dev)
            return p


def check_natoms(natoms: Sequence[int], max_atoms: Optional[int] = None, holder: str = "") -> list:
    """natoms as a list of ints: at least one crystal of at least one atom and, with max_atoms, none larger than
    `holder` ("the matcher") stages (ValueError)."""
    nat = [int(n) for n in natoms]
    if not nat or min(nat) < 1:
        raise ValueError("natoms must list at least one crystal of at least one atom")
    if max_atoms is not None and max(nat) > max_atoms:
        raise ValueError(f"{holder} holds at most {max_atoms} atoms per crystal, got {max(nat)}")
    return nat


def check_state(nat: Sequence[int], atom_types, frac_coords, lattices, types_used: bool = True):
    """(N, B, device) of a device state in node order of `nat` (check_natoms' list): atom_types [N] int64,
    frac_coords [N,3] and lattices [B,3,3] float32, contiguous, on one HIP device; ValueError, or RuntimeError for
    a CPU tensor. A leg that does not read atom_types (types_used=False) takes None for it and checks neither its
    dtype nor its device."""
    N, B = sum(nat), len(nat)
    if (atom_types is not None or types_used) and tuple(atom_types.shape) != (N,) or \
            tuple(frac_coords.shape) != (N, 3) or tuple(lattices.shape) != (B, 3, 3):
        raise ValueError("state shapes do not match natoms")
    _lib.require_device(atom_types, frac_coords, lattices)
    ok = frac_coords.dtype == torch.float32 and lattices.dtype == torch.float32
    if not (ok and (not types_used or atom_types.dtype == torch.int64)):
        raise ValueError("the state must be " + ("atom_types int64, " if types_used else "") +
                         "frac_coords / lattices float32")
    dev = frac_coords.device
    if (types_used and atom_types.device != dev) or lattices.device != dev:
        raise ValueError("the state's tensors are on different devices")
    return N, B, dev


def exclude_tensor(exclude, B: int, lists: str):
    """`exclude` (None, a bool / 0-1 array or a tensor) as None or a bool / uint8 tensor [B], still where it was:
    the caller moves it inside its device context. `lists` words the refusal ("the state lists")."""
    if exclude is None:
        return None
    ex = exclude if torch.is_tensor(exclude) else torch.from_numpy(np.ascontiguousarray(np.asarray(exclude)))
    if tuple(ex.shape) != (B,):
        raise ValueError(f"exclude has shape {tuple(ex.shape)}, {lists} {B} crystals")
    if ex.dtype not in (torch.bool, torch.uint8):
        raise ValueError("exclude must be bool or uint8")
    return ex
