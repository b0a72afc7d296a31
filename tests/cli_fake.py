"""What stands in for `LMInferer` under `lungmask_amd.__main__.main` in the host tests of the command line (a plain module, no
test): the labels are a fixed mask, every product comes from the emulated engine.  A test sets `FakeInferer.engine` and
`FakeInferer.labels` and puts the class in the place of `cli.LMInferer`."""
from lungmask_amd import components as cp
from lungmask_amd import filters as flt
from lungmask_amd import mesh as lmmesh
from lungmask_amd import skeleton as sk
from lungmask_amd import stats as lmstats
from lungmask_amd import vessels as vs


class FakeInferer:
    engine = None
    labels = None
    modelname = "R231"

    def __init__(self, *a, **kw):
        pass

    def _names(self):
        return lmstats.label_names("R231", 3)

    def apply(self, image):
        return self.labels.copy()

    def apply_denoised(self, image, method="median", size=3, sigma_mm=None):
        res = self.labels.copy()
        if method == "median":
            return res, flt.median(image, size, labels=res, engine=self.engine)
        return res, flt.gaussian(image, sigma_mm, labels=res, engine=self.engine)

    def apply_with_clusters(self, image, threshold=-950, hu_range=None, connectivity=6):
        res = self.labels.copy()
        return res, cp.cluster_analysis(image, res, threshold, hu_range, connectivity, names=self._names(), engine=self.engine)

    def apply_with_stats(self, image):
        res = self.labels.copy()
        return res, lmstats.label_statistics(image, res, names=self._names(), engine=self.engine, n_labels=3)

    def apply_with_vessels(self, image, **kw):
        return self.labels.copy(), vs.vessel_result(image, self.labels, names=self._names(), engine=self.engine, **kw)

    def apply_with_vessel_tree(self, image, **kw):
        return self.labels.copy(), sk.vessel_tree(image, self.labels, names=self._names(), engine=self.engine, **kw)

    def apply_mesh(self, image, per_label=True, smooth=0):
        res = self.labels.copy()
        return res, lmmesh.extract_surfaces(image.like(res), per_label=per_label, smooth=smooth, engine=self.engine)
