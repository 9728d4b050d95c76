"""``crimp`` import name for the MI355X build: ``from crimp.periodsearch import PeriodSearch`` and every other
``crimp.<module>`` this build provides resolve to the drop-in module ``crimp_amd.<module>`` (the same module object,
so state and classes are shared): the photon hot path (``calcphase``, ``periodsearch``, ``templatemodels``,
``measureToAs``, ``pulseprofile``, ``eventfile``, ``timfile``, ...), the timing-model fits of the ToAs
(``fit_toas``, ``utilities_fittoas``, ``get_local_ephem``, ``plot_local_ephem``) and the event simulator
(``simulatemodulatedlc``). Modules the build does not provide (``diagnoseToAs``, ``merge_overlapping_timfiles``) raise
ImportError as a missing module would. The
pulse-profile plots are provided as ``crimp_amd.plot_pps`` (and the ``pulseprofile_plots`` script) only, as
tests/test_capi_and_host.py::test_crimp_import_name_and_entry_points pins it (``crimp.plot_pps`` raises)."""
import importlib
import importlib.abc
import importlib.util
import sys

from crimp_amd import __version__  # noqa: F401

NOT_ALIASED = ("plot_pps",)  # imported under its own name only


class _AliasFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, fullname, path, target=None):
        if not fullname.startswith("crimp.") or fullname.count(".") != 1:
            return None
        name = fullname.split(".", 1)[1]
        if name in NOT_ALIASED or importlib.util.find_spec("crimp_amd." + name) is None:
            return None
        return importlib.util.spec_from_loader(fullname, self)

    def create_module(self, spec):
        return importlib.import_module("crimp_amd." + spec.name.split(".", 1)[1])

    def exec_module(self, module):
        pass


if not any(isinstance(f, _AliasFinder) for f in sys.meta_path):
    sys.meta_path.insert(0, _AliasFinder())
