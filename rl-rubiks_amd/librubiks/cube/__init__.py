# The public surface is the module-level function API, used as `from librubiks import cube`
# (reference librubiks/cube/__init__.py:2).
from .cube import *  # noqa: F401,F403
from .cube import Cube, scramble_batch, sequence_scrambler_device  # noqa: F401
from .device import DeviceCubes  # noqa: F401
from .device import DeviceCubes686  # noqa: F401
from . import cube686  # noqa: F401  (the reference's 6x8x6 representation, as a namespace of its own)
