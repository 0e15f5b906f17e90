"""TEST INFRASTRUCTURE: the exact CPU twin of a backend that keeps the W8A16 and PEG recipes on the integer route at any token
count (options.INT8_RAGGED_RECIPES).

Nothing is computed here that the other twins do not compute already: `ExactBackend.linear_i8_cls`, `linear_i16x8` and
`quantize_hilo` take any row count (they are the formulas the kernel tests use as reference, row by row), PackedTwin brings the
ragged and variable-length attention references, PlaneResidualsTwin and PegIresTwin the tails of the three site-x routes.  The
twin only DECLARES what HipBackend declares -- `PADS_RECIPE_ROWS` -- so the shared host code plans FFN1 of both recipes at a
ragged M.  `NoRecipeRowsTwin` is the same backend without the declaration: the parent commit's.  Nothing outside tests/ imports
this."""
from tests._packed_twin import PackedTwin
from tests._peg_ires_twin import PegIresTwin
from tests._plane_residuals_twin import PlaneResidualsTwin


class NoRecipeRowsTwin(PackedTwin, PlaneResidualsTwin, PegIresTwin):
    """every entry of the route, row tails of the per-tensor plan included (PADS_ROWS), but no PADS_RECIPE_ROWS"""
    name = 'exact-twin-no-recipe-rows'


class RaggedRecipesTwin(NoRecipeRowsTwin):
    name = 'exact-twin-ragged-recipes'
    PADS_RECIPE_ROWS = True
