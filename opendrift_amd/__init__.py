"""opendrift_amd -- MI355X-native particle-advection hot path behind OpenDrift's model/reader API."""
import os as _os

__version__ = '0.2.0'

# Multi-process GPU work on this platform (RCCL, device memory shared between the ranks of a node) needs the dmabuf IPC mode;
# the launch environment normally exports it already.
_os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')


def __getattr__(name):      # the model classes import the device binding: resolved on first use
    if name == 'OpenBerg':
        from .openberg import OpenBerg
        return OpenBerg
    if name == 'ShipDrift':
        from .shipdrift import ShipDrift
        return ShipDrift
    if name == 'RadionuclideDrift':
        from .radionuclides import RadionuclideDrift
        return RadionuclideDrift
    if name == 'LarvalFishExtended':
        from .larvalfish_extended import LarvalFishExtended
        return LarvalFishExtended
    if name == 'PlastDrift':
        from .plastdrift import PlastDrift
        return PlastDrift
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
