"""Attribute-style dict and by-name construction (reference: dnnlib/util.py:41-53, 228-289)."""

import importlib
import sys
from typing import Any


class EasyDict(dict):
    """dict whose items are also attributes: ``d.key`` is ``d['key']``."""

    def __getattr__(self, name: str) -> Any:
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name: str, value: Any) -> None:
        self[name] = value

    def __delattr__(self, name: str) -> None:
        del self[name]


def format_time(seconds) -> str:
    """A duration the way the training log prints it: '42s', '3m 07s', '2h 05m 09s', '1d 03h 20m'."""
    s = int(round(seconds))
    if s < 60:
        return '%ds' % s
    if s < 60 * 60:
        return '%dm %02ds' % (s // 60, s % 60)
    if s < 24 * 60 * 60:
        return '%dh %02dm %02ds' % (s // 3600, s // 60 % 60, s % 60)
    return '%dd %02dh %02dm' % (s // 86400, s // 3600 % 24, s // 60 % 60)


class Logger:
    """Copies everything printed to stdout and stderr into ``file_name`` as well, until ``close()`` (or the end of a ``with``)."""

    def __init__(self, file_name=None, file_mode='w', should_flush=True):
        self.file = open(file_name, file_mode) if file_name is not None else None
        self.should_flush = should_flush
        self.stdout, self.stderr = sys.stdout, sys.stderr
        sys.stdout = sys.stderr = self

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.close()

    def write(self, text):
        if isinstance(text, bytes):
            text = text.decode()
        if not text:
            return
        if self.file is not None:
            self.file.write(text)
        self.stdout.write(text)
        if self.should_flush:
            self.flush()

    def flush(self):
        if self.file is not None:
            self.file.flush()
        self.stdout.flush()

    def close(self):
        self.flush()
        if sys.stdout is self:
            sys.stdout = self.stdout
        if sys.stderr is self:
            sys.stderr = self.stderr
        if self.file is not None:
            self.file.close()
            self.file = None


def get_obj_by_name(name: str) -> Any:
    """Resolve ``'package.module.attr[.attr...]'`` to the Python object it names."""
    parts = name.split('.')
    for split in range(len(parts) - 1, 0, -1):
        try:
            obj = importlib.import_module('.'.join(parts[:split]))
        except ImportError:
            continue
        try:
            for attr in parts[split:]:
                obj = getattr(obj, attr)
            return obj
        except AttributeError:
            continue
    raise ImportError(name)


def call_func_by_name(*args, func_name: str = None, **kwargs) -> Any:
    assert func_name is not None
    func = get_obj_by_name(func_name)
    assert callable(func)
    return func(*args, **kwargs)


def construct_class_by_name(*args, class_name: str = None, **kwargs) -> Any:
    """``construct_class_by_name(class_name='training.networks.Discriminator', **kw)``."""
    return call_func_by_name(*args, func_name=class_name, **kwargs)
