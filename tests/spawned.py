"""Run a GPU test body in a fresh spawned process (tests/test_preprocess_gpu.py, tests/test_inference_tool_gpu.py).

The pytest process of a GPU session is shared by every test that follows: its caching allocators, its pinned host
blocks and its HIP runtime state are what the later tests start from. Tests that only add a feature run their device
work in a child process, so that the rest of the session starts from the state it would have without them."""
import functools
import importlib
import multiprocessing
import traceback

TIMEOUT_S = 900


def _child(module, name, args, kwargs, queue):
    try:
        getattr(importlib.import_module(module), name).__wrapped__(*args, **kwargs)
        queue.put(None)
    except BaseException:                      # noqa: B902 - every failure goes back to the parent as text
        queue.put(traceback.format_exc())


def spawned(fn):
    """decorator: the test runs in a spawned child (same sys.path); its failure is re-raised here with the child's
    traceback. A child that dies or overruns TIMEOUT_S fails the test."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        ctx = multiprocessing.get_context('spawn')
        queue = ctx.SimpleQueue()
        p = ctx.Process(target=_child, args=(fn.__module__, fn.__name__, args, kwargs, queue))
        p.start()
        p.join(TIMEOUT_S)
        if p.is_alive():
            p.kill()
            p.join()
            raise AssertionError('{} did not finish within {} s'.format(fn.__name__, TIMEOUT_S))
        if queue.empty():
            raise AssertionError('{}: the child process ended with exit code {}'.format(fn.__name__, p.exitcode))
        err = queue.get()
        if err is not None:
            raise AssertionError('{} failed in its child process:\n{}'.format(fn.__name__, err))
    return wrapper
