"""The reference's hybrid refractive / diffractive model is not built on this backend."""
raise NotImplementedError("dprox.contrib.optic.doe_model_hybrid is not built on this backend: the DOE model of "
                          "dprox.contrib.optic.doe_model (build_doe_model, RGBCollimator) is")
