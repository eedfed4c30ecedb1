// Pre-included (-include) ahead of the reference's headers by the reference pin build
// (oracle/Makefile, target ref_pin).  It supplies what those headers assume their includer
// brought along: <cassert>, the names of namespace Eigen at global scope
// (CommonUtilities.hpp writes Vector3f unqualified before any using-directive), and a
// dynamic-size Eigen::Matrix for planeFitting, which the pin never calls: the members below
// only have to type-check, and abort if anything ever reaches them.
#pragma once
#include <cassert>
#include <cstdlib>

#include <Eigen/Dense>

namespace Eigen {

constexpr int Dynamic = -1;
enum { ComputeThinU = 4, ComputeThinV = 8 };

template <class S, int R, int C>
struct Matrix;

template <class S>
struct Matrix<S, Dynamic, Dynamic> {
  struct Col {
    Col& operator=(const Vector3f&) { std::abort(); }
  };
  struct Arr {
    Arr& operator-=(S) { std::abort(); }
  };
  struct Row {
    S mean() const { std::abort(); }
    Arr array() { std::abort(); }
  };
  struct U {
    template <int N>
    Vector3f rightCols() const { std::abort(); }
  };
  struct Svd {
    U matrixU() const { std::abort(); }
  };
  Matrix(size_t, size_t) {}
  Col col(size_t) { std::abort(); }
  Row row(size_t) { std::abort(); }
  Svd jacobiSvd(int) { std::abort(); }
};

}  // namespace Eigen

using namespace Eigen;
