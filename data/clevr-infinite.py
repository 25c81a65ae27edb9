"""The reference's import path of the CLEVR-infinite datasets: DataModuleFromConfig names `data.clevr-infinite.Blender3dTrain`,
which `importlib.import_module` resolves to this file although the name is no Python identifier."""
from sgam_neurips22_amd.datasets import Blender3dBase, Blender3dTest, Blender3dTrain, Blender3dValidation  # noqa: F401
