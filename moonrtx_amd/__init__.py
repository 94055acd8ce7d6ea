"""moonrtx_amd -- MI355X (gfx950) renderer backend for MoonRTX's displaced-sphere Moon scene.

Layout (only what the hot path needs):
  csrc/         HIP kernels + the C ABI of include/moonrt.h  -> libmoonrt.so (in-tree)
  _lib.py       ctypes loader (raises if the library is missing: there is no CPU fallback)
  renderer.py   MoonRT, object wrapper over the C ABI: the renderer itself, and through its bases the two stages below
  _calls.py     MoonRTError, DeviceBuffer and the base class of the call classes (_check, _add_stats, config)
  terrain_calls.py   TerrainCalls: the terrain queries, traverses and relief (csrc/mrtx_terrain_api.hip)
  lattice_calls.py   LatticeCalls: regions ... peaks, the calls on per-node tables (csrc/mrtx_lattice_api.hip)
  tkoptix.py    the PlotOptiX-named surface moon_renderer.py drives (`self.rt`)
  scene.py      headless restatement of the scene MoonRenderer pushes (camera, light, Sun disk)
  dist.py       image-tile sharding across GPUs + RCCL gather of the framebuffer
  build.py      hipcc build recipe
"""
__version__ = "0.1.0"
