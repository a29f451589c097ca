"""What the GPU tests of the sparse stack share to show that device tensors never reach a `_cpu` twin."""
from mmdet3d_gaussian_amd import _lib


def refuse_twins(monkeypatch, wanted):
    """every symbol of the library that `wanted(name)` accepts is replaced by a function that raises: a `_cpu` twin called with the
    address of device memory would fault the process"""
    lib = _lib.load()

    def refuse(name):
        def twin(*args):
            raise AssertionError(f'{name} was called for tensors on the device')
        return twin
    for name in _lib.SYMBOLS:
        if wanted(name):
            monkeypatch.setattr(lib, name, refuse(name))
