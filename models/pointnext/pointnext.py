"""Alias of ppt_amd.models.pointnext.pointnext under the reference's module path (models/pointnext/pointnext.py)."""
from ppt_amd.models.pointnext.pointnext import *          # noqa: F401,F403
from ppt_amd.models.pointnext.pointnext import BaseCls, ClsHead, PointNEXT, PointNextEncoder, SetAbstraction  # noqa: F401
