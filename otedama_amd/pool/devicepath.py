"""The pool's device switch: which device a path is configured for, whether it is still in use, and the fall-back to
the CPU when it raises. ``microbatch.ShareBatcher`` (share verification) and ``jobroots.JobRoots`` (a job's fan-out)
each hold one :class:`DevicePath`. Importing this module imports neither torch nor the native extension.

The switch is the process's, per device: a GPU that has faulted for one path is not used again by that path or by
any other in the process (``otedama pool --algorithms a,b`` runs one pool per algorithm on the same device).
"""
from __future__ import annotations

import re

_DEVICE_RE = re.compile(r"^(cpu|cuda:\d+)$")


def valid_device(device: str) -> bool:
    """``""`` (off), ``cpu`` or ``cuda:N``. The one statement of the grammar: config.py and the CLI ask here."""
    return device == "" or bool(_DEVICE_RE.match(device))


# Devices whose path raised in this process. Every path looks here before it chooses the device, on the event loop
# and again on its worker thread, so after one path's device error no other path of the process starts a call on
# that device. Nothing in the package takes a device out again.
_failed_devices: set = set()


def device_failed(device: str) -> bool:
    return device in _failed_devices


def mark_failed(device: str) -> None:
    _failed_devices.add(device)


def forget_device_errors() -> None:
    """For tests that inject a failure: a later test in the same process gets its device back."""
    _failed_devices.clear()


class DevicePath:
    def __init__(self, option: str, device: str):
        """``device``: the value of the pool option ``option`` (``verify_device``, ``job_device``): ``cpu`` or
        ``cuda:N``, anything else is a ``ValueError``."""
        if not valid_device(device) or not device:
            raise ValueError(f"{option} {device!r} must be cpu or cuda:N")
        self.device = device
        self.gpu = device != "cpu"
        self.device_errors = 0

    @property
    def on(self) -> bool:
        return self.gpu and not device_failed(self.device)

    @property
    def enabled(self) -> bool:
        """For the stats: the configured path is in use (False once a device error, of this path or of another path
        of the process on the same device, has turned the GPU path off)."""
        return self.on or not self.gpu

    def run(self, on_device, on_cpu):
        """On the worker thread, for work the event loop chose the device for: ``(result, ran on the device, device
        error)``. Another path may have failed since the loop looked, so the switch is read again. Whatever
        ``on_device()`` raises is counted, turns the device off for the process, and ``on_cpu()`` answers instead."""
        if not self.on:
            return on_cpu(), False, None
        try:
            return on_device(), True, None
        except Exception as exc:  # noqa: BLE001 - whatever the device path raised, the work is still answered
            mark_failed(self.device)
            self.device_errors += 1
            return on_cpu(), False, exc
