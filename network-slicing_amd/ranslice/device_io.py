"""DeviceArray: a typed view of device memory that a handle owns (rs_get_device_view) or that the caller brought.

It carries no framework: `__cuda_array_interface__` (version 3) is what torch, cupy and numba read to wrap the memory in
place (`torch.as_tensor(view['obs_norm'], device='cuda')` shares it; on ROCm the protocol keeps its CUDA name), and
get() / set() move whole arrays across the C ABI (rs_device_copy, on the owner handle's stream) for hosts without one.
"""
import ctypes as C

import numpy as np

_TYPESTR = {np.dtype(np.float32): '<f4', np.dtype(np.int32): '<i4', np.dtype(np.int64): '<i8',
            np.dtype(np.float64): '<f8', np.dtype(np.int16): '<i2'}


class DeviceArray:
    """pointer + shape + dtype of a C-contiguous device array, and the environment (VecRanSlice) whose handle owns it"""

    def __init__(self, ptr, shape, dtype, owner=None):
        self.ptr = int(ptr)
        self.shape = tuple(int(x) for x in shape)
        self.dtype = np.dtype(dtype)
        if self.dtype not in _TYPESTR:
            raise ValueError('DeviceArray: unsupported dtype %s' % self.dtype)
        self.owner = owner

    @property
    def size(self):
        n = 1
        for x in self.shape:
            n *= x
        return n

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    def data_ptr(self):
        return self.ptr

    @property
    def __cuda_array_interface__(self):
        # stream omitted: consumers do not synchronise on import; ordering is rs_step_device's / stream_join's business
        return {'shape': self.shape, 'typestr': _TYPESTR[self.dtype], 'data': (self.ptr, False), 'version': 3,
                'strides': None}

    def _handle(self):
        if self.owner is None or not getattr(self.owner, 'h', None):
            raise ValueError('DeviceArray: no live owner handle to copy through')
        return self.owner

    def get(self):
        """the array on the host, after everything queued on the owner's stream so far"""
        env = self._handle()
        out = np.empty(self.shape, dtype=self.dtype)
        env._check(env.L.rs_device_copy(env.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), self.nbytes, 0))
        return out

    def set(self, array):
        """host -> device on the owner's stream (ordered before its next step)"""
        env = self._handle()
        a = np.ascontiguousarray(array, dtype=self.dtype)
        if a.shape != self.shape:
            raise ValueError('DeviceArray.set: shape %s does not match %s' % (a.shape, self.shape))
        env._check(env.L.rs_device_copy(env.h, C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), self.nbytes, 1))
        return self

    def __repr__(self):
        return 'DeviceArray(0x%x, shape=%s, dtype=%s)' % (self.ptr, self.shape, self.dtype)


def describe(actions):
    """(pointer, shape or None, dtype or None) of what step_device accepts: a DeviceArray, an object with
    __cuda_array_interface__ (contiguity checked), one with data_ptr() (a torch tensor), or a plain int pointer"""
    if isinstance(actions, DeviceArray):
        return actions.ptr, actions.shape, actions.dtype
    cai = getattr(actions, '__cuda_array_interface__', None)
    if cai is not None:
        shape = tuple(int(x) for x in cai['shape'])
        dtype = np.dtype(cai['typestr'])
        strides = cai.get('strides')
        if strides is not None:
            want, acc = [], dtype.itemsize
            for n in reversed(shape):
                want.append(acc)
                acc *= n
            if any(n > 1 and int(s) != w for n, s, w in zip(reversed(shape), reversed(tuple(strides)), want)):
                raise ValueError('step_device: the action array is not C-contiguous')
        return int(cai['data'][0]), shape, dtype
    if hasattr(actions, 'data_ptr'):
        if hasattr(actions, 'is_contiguous') and not actions.is_contiguous():
            raise ValueError('step_device: the action tensor is not contiguous')
        shape = tuple(int(x) for x in actions.shape) if hasattr(actions, 'shape') else None
        dtype = None
        name = str(getattr(actions, 'dtype', '')).split('.')[-1]
        if name in ('float32', 'int32', 'int64', 'float64', 'int16'):
            dtype = np.dtype(name)
        return int(actions.data_ptr()), shape, dtype
    if isinstance(actions, (int, np.integer)):
        return int(actions), None, None
    raise ValueError('step_device: expected a DeviceArray, an object with __cuda_array_interface__ or data_ptr(), or a pointer')
