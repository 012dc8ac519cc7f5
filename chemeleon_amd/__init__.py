"""chemeleon_amd — MI355X-native (gfx950) implementation of Chemeleon's
reverse-diffusion sampling path, a drop-in for `chemeleon.Chemeleon` /
`chemeleon.modules.cspnet.CSPNet` on that path.

    from chemeleon_amd import Chemeleon
"""

from chemeleon_amd.modules.chemeleon import Chemeleon  # noqa: F401
from chemeleon_amd.modules.cspnet import CSPNet, DECODER_OUTPUTS  # noqa: F401
from chemeleon_amd.constraints import Constraint  # noqa: F401
from chemeleon_amd.screening import Screen, ScreenReport, screen_states  # noqa: F401
from chemeleon_amd.dedup import (Dedup, DedupReport, Fingerprints, dedup_states, fingerprint_states,  # noqa: F401
                                 group_fingerprints)
from chemeleon_amd.cell import Cell, CellReport, cell_states, reduce_states  # noqa: F401
from chemeleon_amd.symmetry import CRYSTAL_SYSTEMS, Symmetry, SymmetryReport, symmetry_states  # noqa: F401
from chemeleon_amd.primitive import Primitive, PrimitiveReport, primitive_states  # noqa: F401
from chemeleon_amd.match import Match, MatchReport, Reference, match_states  # noqa: F401
from chemeleon_amd.match_group import MatchDedup, MatchGroupReport, match_group_states  # noqa: F401
from chemeleon_amd.match_set import MatchSet, MatchSetReport, ReferenceSet, match_set_states  # noqa: F401

__all__ = ["Chemeleon", "CSPNet", "DECODER_OUTPUTS", "Constraint", "Screen", "ScreenReport", "screen_states",
           "Dedup", "DedupReport", "Fingerprints", "dedup_states", "fingerprint_states", "group_fingerprints",
           "Cell", "CellReport", "cell_states", "reduce_states", "CRYSTAL_SYSTEMS", "Symmetry", "SymmetryReport",
           "symmetry_states", "Primitive", "PrimitiveReport", "primitive_states", "Match", "MatchReport", "Reference",
           "match_states", "MatchDedup", "MatchGroupReport", "match_group_states", "MatchSet",
           "MatchSetReport", "ReferenceSet", "match_set_states"]
__version__ = "0.1.0"
