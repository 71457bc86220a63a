"""pyratslam_amd -- the pyratslam hot path (pose-cell network step and
view-template matcher) as hand-written HIP kernels for AMD Instinct MI355X
(gfx950), behind a C ABI (``include/ratslam_abi.h``) and drop-in Python classes
with the reference's API (``/root/reference/ratslam/posecell_network.py``,
``view_templates.py``).

    from pyratslam_amd import PoseCellNetwork, ViewTemplates
"""
from .linked_experience_map import LinkedExperienceMap, NumpyLinkedExperienceMap  # noqa: F401
from .pc_peak import numpy_peak_sums, peak_tables, pose_from_sums  # noqa: F401
from .pose_ensemble import PoseCellEnsemble  # noqa: F401
from .posecell_network import PoseCellNetwork  # noqa: F401
from .view_templates import (ShardedViewTemplates, ViewTemplate, ViewTemplates, numpy_offset_profile,  # noqa: F401
                             normalise_u8, numpy_sad_u8_scores, refine_offset)
from .visual_odometer import NumpyVisualOdometer, SimpleVisualOdometer  # noqa: F401

__version__ = '0.1.0'
