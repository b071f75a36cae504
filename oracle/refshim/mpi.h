// Stand-in for <mpi.h> in the CPU build of the reference: a world of one rank.
#pragma once
#include <cstring>

typedef int MPI_Comm;
typedef int MPI_Datatype;
typedef int MPI_Op;
#define MPI_COMM_WORLD 0
#define MPI_FLOAT 1
#define MPI_SUM 1
#define MPI_SUCCESS 0

inline int MPI_Init(int *, char ***) { return MPI_SUCCESS; }
inline int MPI_Finalize() { return MPI_SUCCESS; }
inline int MPI_Comm_size(MPI_Comm, int *size) {
  *size = 1;
  return MPI_SUCCESS;
}
inline int MPI_Comm_rank(MPI_Comm, int *rank) {
  *rank = 0;
  return MPI_SUCCESS;
}
// One rank: the sum over ranks is the rank's own buffer (MPI_FLOAT only).
inline int MPI_Reduce(const void *send, void *recv, int count, MPI_Datatype, MPI_Op, int, MPI_Comm) {
  std::memcpy(recv, send, sizeof(float) * (size_t)count);
  return MPI_SUCCESS;
}
