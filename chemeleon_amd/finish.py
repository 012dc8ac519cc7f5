"""The tail of Chemeleon.sample(): the optional legs that run on the finished state on the device (the screen,
chemeleon_amd.screening; the primitive cell, chemeleon_amd.primitive; the cell, chemeleon_amd.cell; the symmetry, chemeleon_amd.symmetry; the matching,
chemeleon_amd.match; the search of a reference set, chemeleon_amd.match_set; the grouping, chemeleon_amd.dedup or, with a MatchDedup, chemeleon_amd.match_group), in one function. screened_atoms, deduped_atoms and finished_atoms of those modules call it."""

from typing import Sequence

import numpy as np


def finish_atoms(natoms: Sequence[int], atom_types, frac_coords, lattices, screen=None, cell=None, symmetry=None,
                 dedup=None, match=None, primitive=None, search=None):
    """(structures, reports): the tail of sample() with any of its optional legs, in this order: the screen,
    the primitive cell (which replaces the state for every leg after it and for the structures returned),
    the cell, the symmetry, the matching, the search of a reference set, then the grouping, from which the failures of
    the legs before it (a screen flag; a required lattice system or crystal system not met; with match.require, no
    match; with search.require, a sample that is not "known" / not "novel") are excluded. Only the structures that pass (with dedup:
    one representative per group) are copied and converted (in their reduced cells with cell.reduce), each with
    atoms.info["screen"] / ["primitive"] / ["cell"] / ["symmetry"] / ["match"] / ["search"] / ["dedup"] for the legs that ran.
    `reports` is a dict with the report of each leg that ran under the same names."""
    from chemeleon_amd.screening import screen_states, selected_atoms
    nat = [int(n) for n in natoms]
    reports = {}
    failed = None
    if screen is not None:
        reports["screen"] = screen_states(nat, atom_types, frac_coords, lattices, screen)
        failed = ~reports["screen"].valid
    if primitive is not None:  # (from here on the state is the primitive cells': the crystals keep their indices)
        from chemeleon_amd.primitive import primitive_states
        nat, atom_types, frac_coords, lattices, reports["primitive"] = primitive_states(
            nat, atom_types, frac_coords, lattices, primitive)
    x, lat = frac_coords, lattices
    if cell is not None:
        from chemeleon_amd.cell import _run
        x_r, lat_r, reports["cell"] = _run(nat, atom_types, frac_coords, lattices, cell, cell.reduce)
        failed = reports["cell"].mismatch.copy() if failed is None else failed | reports["cell"].mismatch
        if cell.reduce:
            x, lat = x_r, lat_r
    if symmetry is not None:
        from chemeleon_amd.symmetry import symmetry_states
        reports["symmetry"] = symmetry_states(nat, atom_types, frac_coords, lattices, symmetry)
        failed = reports["symmetry"].mismatch.copy() if failed is None else failed | reports["symmetry"].mismatch
    if match is not None:
        from chemeleon_amd.match import match_states
        reports["match"] = match_states(nat, atom_types, frac_coords, lattices, match)
        if match.require:
            failed = reports["match"].mismatch.copy() if failed is None else failed | reports["match"].mismatch
    if search is not None:
        from chemeleon_amd.match_set import match_set_states
        reports["search"] = match_set_states(nat, atom_types, frac_coords, lattices, search)
        if search.require is not None:
            failed = reports["search"].mismatch.copy() if failed is None else failed | reports["search"].mismatch
    if dedup is not None:
        from chemeleon_amd.match_group import MatchDedup, match_group_states
        if isinstance(dedup, MatchDedup):  # (grouping by matching instead of by fingerprints)
            reports["dedup"] = match_group_states(nat, atom_types, frac_coords, lattices, dedup, failed)
        else:
            from chemeleon_amd.dedup import dedup_states
            reports["dedup"] = dedup_states(nat, atom_types, frac_coords, lattices, dedup, failed)
        keep = np.flatnonzero(reports["dedup"].representative).tolist()
    elif failed is not None:
        keep = np.flatnonzero(~failed).tolist()
    else:
        keep = list(range(len(nat)))
    if not keep:
        return [], reports
    atoms = selected_atoms(nat, atom_types, x, lat, keep)
    for at, g in zip(atoms, keep):
        if "screen" in reports:
            at.info["screen"] = dict(reports["screen"].record(g), index=g)
        if "primitive" in reports:
            at.info["primitive"] = dict(reports["primitive"].record(g), index=g)
        if "cell" in reports:
            at.info["cell"] = dict(reports["cell"].record(g), index=g, reduced=cell.reduce)
        if "symmetry" in reports:
            at.info["symmetry"] = dict(reports["symmetry"].record(g), index=g)
        if "match" in reports:
            at.info["match"] = dict(reports["match"].record(g), index=g)
        if "search" in reports:
            at.info["search"] = dict(reports["search"].record(g), index=g)
        if "dedup" in reports:
            at.info["dedup"] = reports["dedup"].record(g)
    return atoms, reports
