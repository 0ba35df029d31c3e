from .device_actor import DeviceActor, DeviceRollout  # noqa: F401
