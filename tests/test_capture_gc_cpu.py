"""``_lib.capture_without_gc``: a graph capture must not run the cycle collector.  A dead Python cycle can own device resources - an
inference aggregator and its metric families refer to each other, and the aggregator's SHT plan frees device memory in ``__del__`` - and
``torch.cuda.graph`` does not collect on entry, so a collection that lands inside a capture released them there and invalidated it."""
import gc

from ace_amd import _lib


class _Owner:
    """a cycle with a finaliser, as an aggregator with a native plan is"""
    released = []

    def __init__(self, tag):
        self.tag, self.me = tag, self

    def __del__(self):
        _Owner.released.append(self.tag)


def test_dead_cycles_are_released_before_the_body_and_none_inside():
    _Owner.released.clear()
    gc.collect()
    _Owner("before")
    with _lib.capture_without_gc():
        assert _Owner.released == ["before"]          # collected on entry
        assert not gc.isenabled()
        _Owner("inside")
        for _ in range(5):                            # far past every generation's threshold: nothing is collected in here
            junk = [[i] for i in range(200000)]
            del junk
        assert _Owner.released == ["before"]
    assert gc.isenabled()
    gc.collect()
    assert _Owner.released == ["before", "inside"]


def test_the_collector_is_left_as_it_was_found():
    gc.disable()
    try:
        with _lib.capture_without_gc():
            pass
        assert not gc.isenabled()
    finally:
        gc.enable()
    try:
        with _lib.capture_without_gc():
            raise KeyError("x")
    except KeyError:
        pass
    assert gc.isenabled()


def test_an_evaluator_aggregator_is_a_cycle_that_owns_its_plan():
    """the hazard itself, on the host: only the collector frees an aggregator, and with it the plan"""
    import weakref

    from ace_amd.evaluator import InferenceEvaluatorAggregatorConfig
    from test_aggregator_cpu import oracle_sht_factory
    from test_evaluator_aggregator_cpu import case, normalizer
    info = case()[0]
    agg = InferenceEvaluatorAggregatorConfig().build(info, 1, 6, normalize=normalizer(), sht_factory=oracle_sht_factory)
    plan = weakref.ref(agg._get_sht())
    gc.collect()
    gc.disable()
    try:
        del agg
        assert plan() is not None
        with _lib.capture_without_gc():
            assert plan() is None
    finally:
        gc.enable()
