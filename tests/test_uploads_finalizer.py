"""The HBM check walks the executor's uploaded host sources while a garbage
collection may finalize one of them: ``_drop_upload`` then pops its entry from
``_uploads``.  The walk must not depend on the dictionary keeping its size."""

import networkx as nx

from dryrun import DryExecutor


class _Upload:
    """Stands for an uploaded DeviceArray whose size query lets a finalizer run."""

    allocated = True

    def __init__(self, on_query):
        self.on_query = on_query

    def device_bytes(self):
        self.on_query()
        return 256


def test_hbm_check_survives_an_upload_dropped_during_the_walk(built):
    from cubed_amd.runtime.executors.gpu import _drop_upload
    import weakref

    ex = DryExecutor()
    ref = weakref.ref(ex)
    # the first entry's query drops the last one, as the finalizer of a collected source array does
    ex._uploads[1] = _Upload(lambda: _drop_upload(ref, 3))
    ex._uploads[2] = _Upload(lambda: None)
    ex._uploads[3] = _Upload(lambda: None)
    ex._check_hbm(nx.DiGraph())
    assert sorted(ex._uploads) == [1, 2]
    # the entries present when the walk began were counted
    assert ex._resident_bytes == 3 * 256
