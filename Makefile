# libgfslam (HIP, gfx950) + the CPU oracle (test infrastructure).
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
ARCH    ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
           -fhip-fp32-correctly-rounded-divide-sqrt -Wall -Wno-unused-function
ORCFLAGS = -O3 -fno-tree-vectorize -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function

CSRC    = gf_orb_slam_amd/csrc
HIPSRCS = $(wildcard $(CSRC)/*.hip)
HIPOBJS = $(patsubst $(CSRC)/%.hip,build/%.o,$(HIPSRCS))
CPPSRCS = $(wildcard $(CSRC)/*.cpp)
CPPOBJS = $(patsubst $(CSRC)/%.cpp,build/%.cpp.o,$(CPPSRCS))
HDRS    = $(wildcard $(CSRC)/*.h) include/gfslam/abi.h include/gfslam/orbslam.h
LIB     = gf_orb_slam_amd/libgfslam.so

ORCSRCS = $(wildcard oracle/*.cpp)
ORCLIB  = oracle/liboracle.so

all: $(LIB) $(ORCLIB)

build/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

build/%.cpp.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p build
	$(CXX) -O3 -fno-tree-vectorize -std=c++17 -fPIC -ffp-contract=off -Wall -c $< -o $@

$(LIB): $(HIPOBJS) $(CPPOBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -L/opt/rocm/lib -lrccl -o $@

$(ORCLIB): $(ORCSRCS) $(wildcard oracle/*.h) $(CSRC)/orb_pattern.h $(CSRC)/select.h $(CSRC)/libm_sincosf.h include/gfslam/abi.h
	$(CXX) $(ORCFLAGS) -shared $(ORCSRCS) -o $@ -lpthread

# timing copy of the oracle for bench.py's cpu_baseline: vectorisation on,
# AVX2-class target (portable to the GPU node's host), same arithmetic order
ORCFAST = oracle/liboracle_fast.so
all: $(ORCFAST)
$(ORCFAST): $(ORCSRCS) $(wildcard oracle/*.h) $(CSRC)/orb_pattern.h $(CSRC)/select.h $(CSRC)/libm_sincosf.h include/gfslam/abi.h
	$(CXX) -O3 -march=x86-64-v3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function -shared $(ORCSRCS) -o $@ -lpthread

clean:
	rm -rf build $(LIB) $(ORCLIB) $(ORCFAST)

.PHONY: all clean

SELCHECK = tests/helpers/libselcheck.so
all: $(SELCHECK)
$(SELCHECK): tests/helpers/select_check.cpp $(CSRC)/select.h
	$(CXX) -O2 -std=c++17 -fPIC -shared $< -o $@

# the tests' CPU restatement of Sim3Solver (tests/test_sim3.py): oracle-style
# flags, no vectorisation, no contraction
SIM3REF = tests/helpers/libsim3ref.so
all: $(SIM3REF)
$(SIM3REF): tests/helpers/sim3_ref.cpp include/gfslam/abi.h
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of OptimizeSim3 and of the Sim3 projection search
# (tests/test_sim3_optimize.py), same flags
SIM3OPTREF = tests/helpers/libsim3optref.so
all: $(SIM3OPTREF)
$(SIM3OPTREF): tests/helpers/sim3opt_ref.cpp include/gfslam/abi.h
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of OptimizeEssentialGraph
# (tests/test_essgraph_cpu.py, tests/test_essgraph_gpu.py), same flags
ESSGRAPHREF = tests/helpers/libessgraphref.so
all: $(ESSGRAPHREF)
$(ESSGRAPHREF): tests/helpers/essgraph_ref.cpp include/gfslam/abi.h
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of Fuse(pKF, Scw, ...), SearchAndFuse and
# MapPoint::Replace (tests/test_loopfuse_cpu.py, tests/test_loopfuse_gpu.py),
# same flags
LOOPFUSEREF = tests/helpers/libloopfuseref.so
all: $(LOOPFUSEREF)
$(LOOPFUSEREF): tests/helpers/loopfuse_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of KeyFrameDatabase::add / erase /
# DetectLoopCandidates and LoopClosing::DetectLoop
# (tests/test_loopdetect_cpu.py, tests/test_loopdetect_gpu.py), same flags
LOOPDETECTREF = tests/helpers/libloopdetectref.so
all: $(LOOPDETECTREF)
$(LOOPDETECTREF): tests/helpers/loopdetect_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of LocalMapping::CreateNewMapPoints, ComputeF12,
# KeyFrame::ComputeSceneMedianDepth and MapPointCulling
# (tests/test_localmap_cpu.py, tests/test_localmap_gpu.py), same flags
LOCALMAPREF = tests/helpers/liblocalmapref.so
all: $(LOCALMAPREF)
$(LOCALMAPREF): tests/helpers/localmap_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of LocalMapping::SearchInNeighbors, plain
# ORBmatcher::Fuse, MapPoint::Replace / UpdateNormalAndDepth and
# KeyFrame::UpdateConnections (tests/test_neighbors_cpu.py,
# tests/test_neighbors_gpu.py), same flags
NEIGHBORSREF = tests/helpers/libneighborsref.so
all: $(NEIGHBORSREF)
$(NEIGHBORSREF): tests/helpers/neighbors_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of LocalMapping::KeyFrameCulling,
# KeyFrame::SetBadFlag / EraseConnection / SetErase and
# MapPoint::EraseObservation / SetBadFlag (tests/test_kfcull_cpu.py,
# tests/test_kfcull_gpu.py), same flags
KFCULLREF = tests/helpers/libkfcullref.so
all: $(KFCULLREF)
$(KFCULLREF): tests/helpers/kfcull_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of Optimizer::LocalBundleAdjustment on a map: the
# gather, the graph and the write-back, without the solver
# (tests/test_lbamap_cpu.py, tests/test_lbamap_gpu.py), same flags
LBAMAPREF = tests/helpers/liblbamapref.so
all: $(LBAMAPREF)
$(LBAMAPREF): tests/helpers/lbamap_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of KeyFrame::UpdateConnections / AddConnection and
# of the index state of LocalMapping::ProcessNewKeyFrame
# (tests/test_covis_cpu.py, tests/test_covis_gpu.py), same flags
COVISREF = tests/helpers/libcovisref.so
all: $(COVISREF)
$(COVISREF): tests/helpers/covis_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of the resident map tables' journal apply and
# regrow (tests/test_maptables_cpu.py, tests/test_maptables_gpu.py), same flags
MAPTABLESREF = tests/helpers/libmaptablesref.so
all: $(MAPTABLESREF)
$(MAPTABLESREF): tests/helpers/maptables_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of Tracking::CreateInitialMap around the solver:
# the map's points and graph, and the median-depth scaling
# (tests/test_initmap_cpu.py, tests/test_initmap_gpu.py), same flags
INITMAPREF = tests/helpers/libinitmapref.so
all: $(INITMAPREF)
$(INITMAPREF): tests/helpers/initmap_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of ORBmatcher::SearchForInitialization over
# Frame::GetFeaturesInArea and of the gate of Tracking::Initialize
# (tests/test_searchinit_cpu.py, tests/test_searchinit_gpu.py,
# tests/test_tracking_init_gpu.py), same flags
SEARCHINITREF = tests/helpers/libsearchinitref.so
all: $(SEARCHINITREF)
$(SEARCHINITREF): tests/helpers/searchinit_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of Tracking::NeedNewKeyFrame / CreateNewKeyFrame,
# KeyFrame::TrackedMapPoints, the KeyFrame snapshot and the hand-over to
# LocalMapping (tests/test_newkeyframe_cpu.py, tests/test_newkeyframe_gpu.py),
# same flags
NEWKFREF = tests/helpers/libnewkeyframeref.so
all: $(NEWKFREF)
$(NEWKFREF): tests/helpers/newkeyframe_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of gf_frontend_update_maps: a map delta's verdict
# and the delta applied to one stream's flat arrays
# (tests/test_mapupdate_cpu.py, tests/test_mapupdate_gpu.py), same flags
MAPUPDATEREF = tests/helpers/libmapupdateref.so
all: $(MAPUPDATEREF)
$(MAPUPDATEREF): tests/helpers/mapupdate_ref.cpp include/gfslam/abi.h
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of gf_frontend_compact_maps: a request's verdict,
# the pins and the restriction of one stream's flat arrays
# (tests/test_mapcompact_cpu.py, tests/test_mapcompact_gpu.py), same flags
MAPCOMPACTREF = tests/helpers/libmapcompactref.so
all: $(MAPCOMPACTREF)
$(MAPCOMPACTREF): tests/helpers/mapcompact_ref.cpp
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# the tests' CPU restatement of the relocalisation database that grows:
# KeyFrameDatabase::add into the packed inverted file, the append of database
# rows and the verdicts (tests/test_kfdb_grow_cpu.py, tests/test_kfdb_grow_gpu.py),
# same flags
KFDBREF = tests/helpers/libkfdbref.so
all: $(KFDBREF)
$(KFDBREF): tests/helpers/kfdb_ref.cpp include/gfslam/abi.h
	$(CXX) $(ORCFLAGS) -shared $< -o $@

# C++ drop-in layer driver (tests/test_dropin_gpu.py runs it on the GPU box)
DROPIN = tests/cpp/dropin_frontend
all: $(DROPIN)
$(DROPIN): tests/cpp/dropin_frontend.cpp include/gfslam/orbslam.h include/gfslam/abi.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude $< -Lgf_orb_slam_amd -lgfslam -Wl,-rpath,'$$ORIGIN/../../gf_orb_slam_amd' -o $@

# C-ABI-only caller: batched front-end sequence + local BA (tests/test_dropin_gpu.py)
SEQDRV = tests/cpp/sequence_driver
all: $(SEQDRV)
$(SEQDRV): tests/cpp/sequence_driver.cpp include/gfslam/orbslam.h include/gfslam/abi.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude $< -Lgf_orb_slam_amd -lgfslam -Wl,-rpath,'$$ORIGIN/../../gf_orb_slam_amd' -o $@

# drop-in Optimizer::BundleAdjustment caller (tests/test_initmap_dropin_gpu.py)
BADRV = tests/cpp/ba_driver
all: $(BADRV)
$(BADRV): tests/cpp/ba_driver.cpp include/gfslam/orbslam.h include/gfslam/abi.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude $< -Lgf_orb_slam_amd -lgfslam -Wl,-rpath,'$$ORIGIN/../../gf_orb_slam_amd' -o $@

# drop-in ORBmatcher::SearchForInitialization caller (tests/test_searchinit_dropin_gpu.py)
SIDRV = tests/cpp/searchinit_driver
all: $(SIDRV)
$(SIDRV): tests/cpp/searchinit_driver.cpp include/gfslam/orbslam.h include/gfslam/abi.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude $< -Lgf_orb_slam_amd -lgfslam -Wl,-rpath,'$$ORIGIN/../../gf_orb_slam_amd' -o $@

# diagnostic build: k_active_match phase stamps (scripts/am_stamps.py), never the product
STAMPLIB = gf_orb_slam_amd/diag/libgfslam_am.so
stamp: $(STAMPLIB)
build/stamp/gf.o: $(CSRC)/gf.hip $(HDRS)
	@mkdir -p build/stamp
	$(HIPCC) $(HIPFLAGS) -DGF_AM_STAMP -c $< -o $@
$(STAMPLIB): build/stamp/gf.o $(filter-out build/gf.o,$(HIPOBJS)) $(CPPOBJS) | gf_orb_slam_amd/diag
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -L/opt/rocm/lib -lrccl -o $@
gf_orb_slam_amd/diag:
	mkdir -p $@
.PHONY: stamp
