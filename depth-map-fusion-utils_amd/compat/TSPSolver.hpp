// TSPSolver.hpp — drop-in for the reference's tour solvers (include/TSPSolver.hpp): the classes
// its planners' run_tsp builds over a cost map (tests/CameraPathGen.cpp, CameraMotionTSP.cpp,
// CalibrationPathGen.cpp, ArtificialLocations.cpp, TSPSolver.cpp) -- TSP::NearestNeighborSearch,
// then TSP::TwoOptSearch from its path.  The members keep the reference's names; the two solve()
// run on the GPU (dmf_tour_nearest_neighbour, dmf_tour_two_opt) on the device of
// dmf_compat::service_volume().  The reference's 2-opt rebuilds and re-sums the path for every
// candidate; the engine returns the same path from prefix sums.  Differences, all where the
// reference is undefined or aborts: a dead end of the nearest-neighbour search (every unvisited
// entry INT_MAX: assert(selected >= 0)) takes the lowest unvisited index; sums are int64 on the
// device, so the paths agree wherever the reference's int sums do not overflow.  The reference's
// include of <nlopt.hpp> is unused and is not repeated; its per-step console print of the
// nearest-neighbour search is dropped.
#pragma once
#include <cassert>
#include <climits>
#include <iostream>
#include <numeric>
#include <stdexcept>
#include <unordered_set>
#include <vector>

#include "Algorithms.hpp"
#include "dmf.h"

namespace TSP {

class GreedySolver {
 public:
  std::vector<std::vector<int>> map_;
  std::vector<int> path_;
  // the path starts as 0, 1, 2, ...
  GreedySolver(std::vector<std::vector<int>>& map) : map_(map), path_(map.size()) {
    std::iota(path_.begin(), path_.end(), 0);
  }
  void printPath() {
    for (int x : path_) std::cout << x << " ";
    std::cout << std::endl;
  }
  std::vector<int> getPath() { return path_; }
  void setPath(std::vector<int>& path) { path_ = path; }
  // the plain int sum over path_, INT_MAX entries included as they are
  int getPathLength() {
    int distance = 0;
    for (size_t i = 1; i < path_.size(); i++) distance += map_[path_[i - 1]][path_[i]];
    return distance;
  }
  // INT_MAX as soon as an edge of `path` is INT_MAX, else the sum
  int getPathLength(std::vector<int>& path) {
    int distance = 0;
    for (size_t i = 1; i < path.size(); i++) {
      const int e = map_[path[i - 1]][path[i]];
      if (e == INT_MAX) return INT_MAX;
      distance += e;
    }
    return distance;
  }

 protected:
  // map_ row-major as the engine takes it; throws unless it is square
  std::vector<int32_t> flatMap() const {
    const size_t V = map_.size();
    std::vector<int32_t> flat(V * V);
    for (size_t a = 0; a < V; ++a) {
      if (map_[a].size() != V) throw std::invalid_argument("TSP: the cost map is not square");
      for (size_t b = 0; b < V; ++b) flat[a * V + b] = map_[a][b];
    }
    return flat;
  }
};

class NearestNeighborSearch : public GreedySolver {
 public:
  NearestNeighborSearch(std::vector<std::vector<int>>& map) : GreedySolver(map) {}
  // From node 0, always on to the unvisited node with the smallest entry below INT_MAX, the lowest
  // index among equals.
  void solve() {
    const std::vector<int32_t> flat = flatMap();
    std::vector<int32_t> path(path_.size());
    dmf_check(dmf_tour_nearest_neighbour(dmf_compat::service_volume(), flat.data(), (int32_t)path.size(), path.data(),
                                         nullptr));
    path_.assign(path.begin(), path.end());
  }
};

class TwoOptSearch : public GreedySolver {
 public:
  TwoOptSearch(std::vector<std::vector<int>>& map) : GreedySolver(map) {}
  // `path` with positions i..k reversed
  std::vector<int> twoOptSwap(std::vector<int> path, int i, int k) {
    std::vector<int> out(path.begin(), path.begin() + i);
    for (int j = k; j >= i; j--) out.push_back(path[j]);
    out.insert(out.end(), path.begin() + k + 1, path.end());
    assert(out.size() == path.size());
    assert(std::unordered_set<int>(out.begin(), out.end()).size() == out.size());
    return out;
  }
  // From path_: the first (i, k), 1 <= i < k, in lexicographic order whose twoOptSwap is strictly
  // shorter by getPathLength(path) replaces the path and the scan restarts; until none is left.
  void solve() {
    const std::vector<int32_t> flat = flatMap();
    std::vector<int32_t> path(path_.begin(), path_.end());
    dmf_check(dmf_tour_two_opt(dmf_compat::service_volume(), flat.data(), (int32_t)path.size(), path.data(), 0, nullptr));
    path_.assign(path.begin(), path.end());
  }
};

}  // namespace TSP
